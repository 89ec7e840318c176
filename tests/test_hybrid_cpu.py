"""CPU: the hybrid conditioning keys of `DiffusionWrapper` (ddpm3d.py:702-763: c_concat joined to x along the channel axis, c_crossattn
as the context) -- the reference's argument handling on a recording stub, the refused keys, the `in_channels = 4 + k` UNet surface,
the argument validation of moca_ncthw_scatter_f16, the 16-channel packing of the first conv, the FIFO refusals and the sensitivity
condition of the hybrid goldens (tools/make_golden_hybrid.py)."""
import ctypes as C
import os
import re
import types

import pytest
import torch
import torch.nn as nn

from helpers import FULL, REDUCED, golden, relerr
from test_unet_gpu import TOL_UNET  # (that module's tests are GPU-marked; importing its constant needs no GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = {"target": "lvdm.modules.networks.openaimodel3d.UNetModel",
        "params": dict(in_channels=8, out_channels=4, model_channels=64, attention_resolutions=[1], num_res_blocks=1, channel_mult=[1],
                       num_head_channels=64, context_dim=64, use_linear=True, temporal_conv=True, use_relative_position=False,
                       temporal_length=16)}


class _Stub(nn.Module):
    """records what DiffusionWrapper hands to the UNet"""

    def __init__(self, in_channels, concat_entry):
        super().__init__()
        self.in_channels = in_channels
        self.calls = []
        if concat_entry:
            self.forward_concat = self._forward_concat

    def forward(self, x, t, **kw):
        self.calls.append(("forward", x, None, kw))
        return x[:, :4]

    def _forward_concat(self, x, c_concat, t, **kw):
        self.calls.append(("forward_concat", x, list(c_concat), kw))
        return x[:, :4]


def _wrapper(key, in_channels=8, concat_entry=True):
    from moca_video_amd import DiffusionWrapper
    w = DiffusionWrapper(TINY, key)
    w.diffusion_model = _Stub(in_channels, concat_entry)
    return w


def _inputs(B=1, ks=(4,)):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 4, 2, 4, 4, generator=g)
    cc = [torch.randn(B, k, 2, 4, 4, generator=g) for k in ks]
    ctx = [torch.randn(B, 77, 64, generator=g), torch.randn(B, 16, 64, generator=g)]
    return x, cc, ctx, torch.tensor([500] * B)


@pytest.mark.parametrize("concat_entry", [True, False])
def test_hybrid_passes_context_pieces_and_drops_fps(concat_entry):
    """ddpm3d.py:713-717: context = cat(c_crossattn, 1); **kwargs (fps) are NOT forwarded; x and the pieces reach the UNet with
    in_channels channels in all -- as pieces through forward_concat where the UNet has it, else as the reference's torch.cat"""
    w = _wrapper("hybrid", concat_entry=concat_entry)
    x, cc, ctx, t = _inputs(ks=(2, 2))
    w(x, t, c_concat=cc, c_crossattn=ctx, fps=torch.tensor([10]), clean_cond=True)
    (kind, gx, pieces, kw), = w.diffusion_model.calls
    assert set(kw) == {"context"} and torch.equal(kw["context"], torch.cat(ctx, 1))
    if concat_entry:
        assert kind == "forward_concat" and gx is x and len(pieces) == 2 and all(a is b for a, b in zip(pieces, cc))
        assert gx.shape[1] + sum(p.shape[1] for p in pieces) == 8
    else:
        assert kind == "forward" and torch.equal(gx, torch.cat([x] + cc, 1))


def test_hybrid_channel_total_is_checked():
    w = _wrapper("hybrid")
    x, cc, ctx, t = _inputs(ks=(4, 1))
    with pytest.raises(ValueError, match="in_channels=8"):
        w(x, t, c_concat=cc, c_crossattn=ctx)
    with pytest.raises(ValueError, match="in_channels=8"):
        w(x, t, c_concat=[cc[1]], c_crossattn=ctx)
    assert not w.diffusion_model.calls


def test_hybrid_variants_keep_the_reference_asserts_and_keywords():
    """:724-759: hybrid-adm needs c_adm (y=), hybrid-time needs s (s=), hybrid-time-adm needs c_adm (s=, y=), hybrid-adm-mask passes
    y=s, mask= and tolerates c_concat=None (xc = x); none of them forwards fps"""
    x, cc, ctx, t = _inputs()
    for key in ("hybrid-adm", "hybrid-time-adm"):
        with pytest.raises(AssertionError):
            _wrapper(key)(x, t, c_concat=cc, c_crossattn=ctx, s=torch.tensor([1]))
    with pytest.raises(AssertionError):
        _wrapper("hybrid-time")(x, t, c_concat=cc, c_crossattn=ctx, c_adm=torch.tensor([1]))
    adm, s, mask = torch.tensor([7]), torch.tensor([3]), torch.ones(1, 1, 2, 4, 4)
    expect = {"hybrid-adm": {"y": adm}, "hybrid-time": {"s": s}, "hybrid-time-adm": {"s": s, "y": adm}, "hybrid-adm-mask": {"y": s, "mask": mask}}
    for key, extra in expect.items():
        w = _wrapper(key)
        w(x, t, c_concat=cc, c_crossattn=ctx, c_adm=adm, s=s, mask=mask, fps=torch.tensor([10]))
        (kind, gx, pieces, kw), = w.diffusion_model.calls
        assert kind == "forward_concat" and gx is x and pieces[0] is cc[0], key
        assert set(kw) == {"context"} | set(extra), key
        assert all(kw[k] is v for k, v in extra.items()), key
    w = _wrapper("hybrid-adm-mask", in_channels=4)
    w(x, t, c_concat=None, c_crossattn=ctx, s=s, mask=mask)
    (kind, gx, pieces, kw), = w.diffusion_model.calls
    assert kind == "forward" and gx is x and kw["y"] is s and kw["mask"] is mask
    with pytest.raises(TypeError):                                  # upstream: `[x] + None`
        _wrapper("hybrid")(x, t, c_concat=None, c_crossattn=ctx)


@pytest.mark.parametrize("key", [None, "concat", "adm", "resblockcond", "concat-time-mask", "concat-adm-mask"])
def test_keys_the_reference_cannot_run_are_refused(key):
    x, cc, ctx, t = _inputs()
    w = _wrapper(key)
    with pytest.raises(NotImplementedError, match=re.escape(repr(key))) as ei:
        w(x, t, c_concat=cc, c_crossattn=ctx)
    assert "reference" in str(ei.value)
    assert not w.diffusion_model.calls


def test_unet_surface_with_concat_channels():
    """in_channels = 4 + k changes the first conv only: 1484 keys, input_blocks.0.0.weight (320, 8, 3, 3); more than 16 is refused"""
    from moca_video_amd import UNetModel
    with torch.device("meta"):
        m = UNetModel(**{**FULL, "in_channels": 8})
        m16 = UNetModel(**{**REDUCED, "in_channels": 16})
    sd = m.state_dict()
    assert len(sd) == 1484 and tuple(sd["input_blocks.0.0.weight"].shape) == (320, 8, 3, 3)
    assert sum(v.numel() for v in sd.values()) == 1413284420 + 320 * 4 * 9
    assert m.in_cpad == 8 and m16.in_cpad == 16 and UNetModel(**{**REDUCED, "in_channels": 9}).in_cpad == 16
    with pytest.raises(NotImplementedError, match="in_channels"):
        UNetModel(**{**FULL, "in_channels": 17})


def test_forward_concat_checks_shapes_before_anything_runs():
    from moca_video_amd import UNetModel
    m = UNetModel(**{**REDUCED, "in_channels": 8})
    x, ctx = torch.zeros(1, 4, 8, 16, 16), torch.zeros(1, 77, 128)
    with pytest.raises(ValueError, match="in_channels=8"):
        m.forward_concat(x, [torch.zeros(1, 3, 8, 16, 16)], torch.tensor([1]), context=ctx)
    with pytest.raises(ValueError, match="batch, frames and size"):
        m.forward_concat(x, [torch.zeros(1, 4, 8, 16, 8)], torch.tensor([1]), context=ctx)
    with pytest.raises(ValueError, match="CUDA"):                   # (right shapes: refused for the device, like forward)
        m.forward_concat(x, [torch.zeros(1, 4, 8, 16, 16)], torch.tensor([1]), context=ctx)


def test_scatter_symbol_and_argument_validation():
    """moca_ncthw_scatter_f16 is declared, exported, mirrored in ctypes, and every bad argument returns MOCA_E_BADARG before a launch
    (no GPU here: a launch would fail differently)"""
    from moca_video_amd import lib
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "moca_hip.h")).read()
    assert re.search(r"\bint\s+moca_ncthw_scatter_f16\s*\(", hdr)
    assert hasattr(l, "moca_ncthw_scatter_f16") and "moca_ncthw_scatter_f16" in lib.SIGNATURES
    f = l.moca_ncthw_scatter_f16
    p = lambda v=64: C.c_void_p(v)
    good = dict(x=p(), f32=1, y=p(), B=1, k=4, T=8, HW=255, Cpad=8, c0=4)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["x"], a["f32"], a["y"], a["B"], a["k"], a["T"], a["HW"], a["Cpad"], a["c0"], None)
    bad = -1
    cases = [dict(x=None), dict(y=None), dict(k=5), dict(c0=5), dict(c0=-1), dict(Cpad=4), dict(Cpad=12), dict(Cpad=32), dict(Cpad=0),
             dict(Cpad=16, c0=13), dict(Cpad=16, c0=8, k=9), dict(B=0), dict(k=0), dict(T=0), dict(HW=0), dict(B=-1), dict(HW=-3),
             dict(y=p(72))]
    for kw in cases:
        assert call(**kw) == bad, kw
        assert call(f32=0, **kw) == bad, kw


def test_pack_conv3x3_with_16_channel_rows():
    """the first conv of a 9..16-channel UNet: [N][(ky, kx, c)] with c zero padded to 16 (K = 144, stored padded to 192)"""
    from moca_video_amd import ops
    g = torch.Generator().manual_seed(5)
    w, b = torch.randn(64, 9, 3, 3, generator=g), torch.randn(64, generator=g)
    p = ops.pack_conv3x3(w, b, cpad=16, device="cpu")
    assert p.K == 144 and p.N == 64 and p.w.shape == (64, 192) and p.w.dtype == torch.float16
    ref = torch.zeros(64, 192, dtype=torch.float16)
    for ky in range(3):
        for kx in range(3):
            ref[:, (ky * 3 + kx) * 16:(ky * 3 + kx) * 16 + 9] = w[:, :, ky, kx].half()
    assert torch.equal(p.w, ref) and torch.equal(p.bias, b)


def _hybrid_dm(key="hybrid", in_channels=8):
    from moca_video_amd import DenoiseModel
    return DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, in_channels=in_channels)},
                        conditioning_key=key)


def test_fifo_paths_refuse_hybrid_conditioning():
    """the reference's FIFO loop never slices c_concat per window: fifo_ddim_sampling, FifoEngine and the multi-prompt loop refuse a
    hybrid model, and a cond that carries c_concat on any model"""
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo import fifo_ddim_sampling, fifo_ddim_sampling_multiprompts
    from moca_video_amd.fifo_graph import FifoEngine
    args = types.SimpleNamespace(num_inference_steps=16, video_length=8, lookahead_denoising=True, num_partitions=2, new_video_length=10)
    ctx = torch.zeros(1, 77, 128)
    cond = {"c_crossattn": [ctx, ctx], "fps": torch.tensor([10])}
    with_cc = dict(cond, c_concat=[torch.zeros(1, 4, 8, 8, 8)])
    plain = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED)})
    lat = torch.zeros(1, 4, 20, 8, 8)
    for dm, c in ((_hybrid_dm(), cond), (_hybrid_dm("hybrid-adm-mask"), cond), (_hybrid_dm(), with_cc), (plain, with_cc)):
        with pytest.raises(NotImplementedError, match="c_concat"):
            FifoEngine(args, dm, None, c, None, 12.0, lat)
        with pytest.raises(NotImplementedError, match="c_concat"):
            fifo_ddim_sampling(args, dm, c, (1, 4, 8, 8, 8), None, cfg_scale=12.0, uc_emb=ctx, latents=lat)
        with pytest.raises(NotImplementedError, match="c_concat"):
            fifo_ddim_sampling_multiprompts(args, dm, c, (1, 4, 8, 8, 8), None, ["a", "b", "4,6"], cfg_scale=12.0, embeds=[ctx, ctx],
                                            uc_emb=ctx, latents=lat)


def test_base_engine_accepts_only_shared_c_concat():
    """fifo_graph.BaseEngine.supported: a hybrid model with the same c_concat tensors in cond and uc; different tensors, a key that
    needs c_adm / s, or c_concat on a crossattn model go to the host-issued path (CPU tensors: `x.is_cuda` is stubbed)"""
    from moca_video_amd.fifo_graph import BaseEngine
    x = types.SimpleNamespace(is_cuda=True, shape=(1, 4, 8, 16, 16))
    ctx, z = torch.zeros(1, 77, 128), torch.zeros(1, 4, 8, 16, 16)
    cond = {"c_concat": [z], "c_crossattn": [ctx], "fps": torch.tensor([10])}
    uc = dict(cond, c_crossattn=[ctx + 1])
    assert BaseEngine.supported(_hybrid_dm(), x, cond, uc, 12.0)
    assert BaseEngine.supported(_hybrid_dm(), x, cond, dict(uc, c_concat=[z[:]], fps=torch.tensor([24])), 12.0)   # a view of the same memory
    assert not BaseEngine.supported(_hybrid_dm(), x, cond, dict(uc, c_concat=[z.clone()]), 12.0)
    assert not BaseEngine.supported(_hybrid_dm(), x, cond, dict(uc, c_concat=[z, z]), 12.0)
    assert not BaseEngine.supported(_hybrid_dm("hybrid-adm"), x, cond, uc, 12.0)
    assert not BaseEngine.supported(_hybrid_dm("hybrid-time"), x, cond, uc, 12.0)
    no_cc = {k: v for k, v in cond.items() if k != "c_concat"}
    assert not BaseEngine.supported(_hybrid_dm(), x, no_cc, dict(no_cc), 12.0)
    # 'hybrid-adm-mask' runs without c_concat -- on a UNet whose in_channels are x's; a wrong channel total of any kind goes to the
    # host-issued path, where the wrapper raises the ValueError that names in_channels
    assert BaseEngine.supported(_hybrid_dm("hybrid-adm-mask", 4), x, no_cc, dict(no_cc), 12.0)
    assert not BaseEngine.supported(_hybrid_dm("hybrid-adm-mask"), x, no_cc, dict(no_cc), 12.0)
    assert not BaseEngine.supported(_hybrid_dm(in_channels=9), x, cond, uc, 12.0)
    two = [z[:, :2], z[:, :2]]
    assert BaseEngine.supported(_hybrid_dm(), x, dict(cond, c_concat=two), dict(uc, c_concat=two), 12.0)
    assert not BaseEngine.supported(_hybrid_dm(), x, dict(cond, c_concat=two[:1]), dict(uc, c_concat=two[:1]), 12.0)
    plain = _hybrid_dm("crossattn", 4)
    assert BaseEngine.supported(plain, x, no_cc, dict(no_cc), 12.0) and not BaseEngine.supported(plain, x, cond, uc, 12.0)


def test_golden_sensitivity_to_c_concat():
    """the cap that keeps the GPU parity tests honest: in case a of hybrid_wrapper.npz, replacing c_concat by zeros moves the REFERENCE's
    output by more than 20 x TOL_UNET (max-norm), so dropped or misplaced concat columns cannot pass under TOL_UNET; case d (fps passed
    in the call) is the reference's case a bit for bit -- the dropped-kwargs quirk, recorded, not assumed"""
    g = golden("hybrid_wrapper")
    moved = relerr(g["a_zero"], g["a"])
    print(f"c_concat -> zeros moves the reference's case a by {moved:.3e} (cap {20 * TOL_UNET:.2e}); c_concat scale {float(g['concat_scale'])}")
    assert moved > 20 * TOL_UNET
    assert g["a"].shape == g["a_zero"].shape == (1, 4, 8, 16, 16)
    assert (g["d"] == g["a"]).all() and float(g["concat_scale"]) >= 1.0
    assert float(golden("hybrid_sample")["concat_scale"]) == float(g["concat_scale"])
