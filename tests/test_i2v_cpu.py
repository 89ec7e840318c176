"""CPU: the image-conditioned UNet surface (use_image_attention=True, the img_cross_attention of attention.py:59-64,82-87,117-124) --
state-dict keys and parameter counts of the reference module tree, YAML instantiation, the C-ABI entry moca_attention_ip_f16 and its
MOCA_E_BADARG refusals (nothing is launched), the ISA of the fused kernel, and the refusals of what the image path does not cover."""
import os
import sys
import types

import pytest
import torch

from helpers import FULL, REDUCED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _meta_unet(**kw):
    from moca_video_amd import UNetModel
    with torch.device("meta"):
        return UNetModel(**kw)


def test_full_width_state_dict_surface():
    """1484 keys of the t2v UNet + 32 attn2.to_{k,v}_ip.weight (16 SpatialTransformer blocks), 1 438 843 460 parameters: the reference's
    own module tree counted with use_image_attention=True"""
    sd = _meta_unet(**dict(FULL, use_image_attention=True)).state_dict()
    sd_t2v = _meta_unet(**FULL).state_dict()
    assert len(sd_t2v) == 1484 and len(sd) == 1516
    assert sum(v.numel() for v in sd.values()) == 1438843460
    extra = sorted(set(sd) - set(sd_t2v))
    assert len(extra) == 32 and not set(sd_t2v) - set(sd)
    for k in extra:
        assert k.endswith(("attn2.to_k_ip.weight", "attn2.to_v_ip.weight")), k
        assert "transformer_blocks.0.attn2" in k and "init_attn" not in k
        assert sd[k].shape[1] == FULL["context_dim"] and sd[k].shape == sd[k.replace("_ip", "")].shape
    # the t2v module tree keeps its attributes: no _ip linears, and image attention off
    assert not any("_ip" in k for k in sd_t2v)


def test_yaml_instantiation_with_image_attention():
    from moca_video_amd import DenoiseModel
    dm = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, use_image_attention=True)})
    unet = dm.model.diffusion_model
    assert unet.use_image_attention
    atts = [m for n, m in unet.named_modules() if n.endswith("attn2")]
    cross = [a for a in atts if not a.is_self]                  # SpatialTransformer attn2; TemporalTransformer attn2 is a self-attention
    assert len(cross) == 16 and len(atts) > len(cross)
    assert all(a.img_cross_attention and a.text_context_len == 77 and a.image_cross_attention_scale == 1.0 for a in cross)
    assert not any(a.img_cross_attention for a in atts if a.is_self)
    assert not hasattr(dm, "embedder")          # the reference branches on hasattr(model, 'embedder') (funcs.py:207)


def test_abi_symbol_and_badarg_refusals():
    """every refusal returns MOCA_E_BADARG before any launch (no GPU here): the pointers below are never dereferenced"""
    import ctypes as C
    from moca_video_amd import lib
    l = lib.load()
    f = l.moca_attention_ip_f16
    P = [C.c_void_p(0x10000 * (i + 1)) for i in range(6)]       # q k v k_ip v_ip out: 16-byte aligned fakes
    good = dict(Bq=2, heads=5, Nq=100, Nt=77, Ni=16, ldq=320, ldk=640, ldv=640, ldk_ip=640, ldv_ip=640, ldo=320, kv_div=1)

    def call(ptrs=P, scale=0.125, ip_scale=1.0, **kw):
        a = dict(good, **kw)
        return f(*ptrs, a["Bq"], a["heads"], a["Nq"], a["Nt"], a["Ni"], a["ldq"], a["ldk"], a["ldv"], a["ldk_ip"], a["ldv_ip"],
                 a["ldo"], a["kv_div"], C.c_float(scale), C.c_float(ip_scale), None)
    bad = -1                                                     # MOCA_E_BADARG
    cases = [dict(Nt=80, Ni=17), dict(Nt=0, Ni=16), dict(Nt=81, Ni=1), dict(Nt=77, Ni=-1), dict(Nt=97, Ni=0), dict(Ni=17),
             dict(ldk_ip=636), dict(ldv_ip=256), dict(ldo=324), dict(ldq=100), dict(kv_div=3), dict(Bq=0), dict(Nq=0)]
    for kw in cases:
        assert call(**kw) == bad, kw
    for i in range(6):
        nul = list(P); nul[i] = None
        assert call(ptrs=nul) == bad, f"null pointer {i}"
        mis = list(P); mis[i] = C.c_void_p(P[i].value + 8)
        assert call(ptrs=mis) == bad, f"misaligned pointer {i}"
    assert call(ip_scale=float("nan")) == bad


def test_isa_of_the_fused_kernel():
    """the two-context instance runs the 77-token kernel's MFMA work (24 per 128-query group) with no scratch, no VGPR spill, no more
    VGPRs (occupancy) than the text-only instance and at most the text-only instance's SGPR spills (to VGPR lanes) + 2"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shutil
    import isa_report
    from moca_video_amd import lib
    if not os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")) or shutil.which("c++filt") is None:
        pytest.skip("llvm-objdump / c++filt not available")
    r = isa_report.analyse(lib.LIB_PATH)
    pick = lambda ip: next(v for k, v in r.items() if "attention_short_kernel" in k and (k.endswith(f"<{ip}>") or f"ILb{int(ip == 'true')}E" in k))
    txt, ip = pick("false"), pick("true")
    assert ip["loop"]["mfma"] == txt["loop"]["mfma"] == 24
    assert ip["mfma_total"] == txt["mfma_total"]
    assert ip["scratch"] == 0 and ip["private_segment_fixed_size"] == 0 and ip["vgpr_spill_count"] == 0
    assert ip["vgpr_count"] <= txt["vgpr_count"] and ip["agpr_count"] == 0
    assert ip["sgpr_spill_count"] <= txt["sgpr_spill_count"] + 2


def test_fifo_refuses_an_image_attention_model():
    """MoCA's 154-token two-prompt context would be split 77 / 77 into text and image by the reference's rule: refused"""
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo import fifo_ddim_sampling
    from moca_video_amd.fifo_graph import FifoEngine
    dm = DenoiseModel({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, use_image_attention=True)})
    args = types.SimpleNamespace(num_inference_steps=16, video_length=8, lookahead_denoising=True, num_partitions=2, new_video_length=10)
    cond = {"c_crossattn": [torch.zeros(1, 77, 128), torch.zeros(1, 77, 128)], "fps": torch.tensor([10])}
    with pytest.raises(NotImplementedError, match="image-attention"):
        FifoEngine(args, dm, None, cond, None, 12.0, torch.zeros(1, 4, 20, 8, 8))
    with pytest.raises(NotImplementedError, match="image-attention"):
        fifo_ddim_sampling(args, dm, cond, (1, 4, 8, 8, 8), None, cfg_scale=12.0, uc_emb=torch.zeros(1, 77, 128),
                           latents=torch.zeros(1, 4, 20, 8, 8))


def test_context_longer_than_the_fused_tile_is_refused():
    """77 text + 16 image tokens fill the key tile: a longer context on an image-attention UNet is a ValueError before anything is
    allocated (the t2v UNet keeps taking 154-token contexts)"""
    from moca_video_amd import UNetModel
    from moca_video_amd.plan import _Plan
    m = UNetModel(**dict(REDUCED, use_image_attention=True))
    for L in (94, 154, ((1, 77), (1, 98))):
        with pytest.raises(ValueError, match="longer than 93"):
            _Plan(m, 1 if isinstance(L, int) else 2, 8, 16, 16, L, torch.float32, torch.device("cpu"))


def test_projector_state_dict_surfaces():
    """the two rows of init_projector (ddpm3d.py:677-687), counted from the reference: Resampler 51 keys / 48 541 696 parameters,
    ImageProjModel 4 keys / 4 200 448"""
    from moca_video_amd import ImageProjModel, Resampler
    with torch.device("meta"):
        res = Resampler(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=1024, ff_mult=4)
        imp = ImageProjModel(clip_extra_context_tokens=4, cross_attention_dim=1024, clip_embeddings_dim=1024)
    sd, si = res.state_dict(), imp.state_dict()
    assert len(sd) == 51 and sum(v.numel() for v in sd.values()) == 48541696
    assert len(si) == 4 and sum(v.numel() for v in si.values()) == 4200448
    assert set(si) == {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
    assert tuple(sd["latents"].shape) == (1, 16, 1024) and tuple(sd["proj_in.weight"].shape) == (1024, 1280)
    for i in range(4):
        for k, shp in (("0.norm1.weight", (1024,)), ("0.norm2.bias", (1024,)), ("0.to_q.weight", (768, 1024)),
                       ("0.to_kv.weight", (1536, 1024)), ("0.to_out.weight", (1024, 768)), ("1.0.weight", (1024,)),
                       ("1.1.weight", (4096, 1024)), ("1.3.weight", (1024, 4096))):
            assert tuple(sd[f"layers.{i}.{k}"].shape) == shp
        assert f"layers.{i}.0.to_q.bias" not in sd and f"layers.{i}.1.1.bias" not in sd
    assert {"proj_out.weight", "proj_out.bias", "norm_out.weight", "norm_out.bias"} <= set(sd)


@pytest.mark.parametrize("finegrained", [True, False])
def test_latent_visual_diffusion_shell(finegrained):
    """the i2v model: YAML-style construction, the projector init_projector picks, the embedder seam (a target that does not import
    leaves it None; get_image_embeds then raises), the projector on precomputed features refuses CPU tensors (no CPU path); the t2v
    DenoiseModel keeps having no `embedder` attribute"""
    from moca_video_amd import DenoiseModel, ImageProjModel, LatentVisualDiffusion, Resampler
    unet_cfg = {"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, context_dim=1024, use_image_attention=True)}
    m = LatentVisualDiffusion({"target": "lvdm.modules.encoders.condition.FrozenOpenCLIPImageEmbedderV2"}, finegrained, unet_config=unet_cfg)
    assert isinstance(m.image_proj_model, Resampler if finegrained else ImageProjModel)
    assert m.model.diffusion_model.use_image_attention and m.embedder is None and hasattr(m, "embedder")
    assert len(m.image_proj_model.state_dict()) == (51 if finegrained else 4)
    with pytest.raises(RuntimeError, match="no image embedder"):
        m.get_image_embeds(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError):
        m.project_image_features(torch.zeros(1, 257, 1280) if finegrained else torch.zeros(1, 1024))
    assert not hasattr(DenoiseModel(unet_cfg), "embedder")


def test_ip_scale_outside_the_bound_is_refused():
    import ctypes as C
    from moca_video_amd import lib
    f = lib.load().moca_attention_ip_f16
    P = [C.c_void_p(0x10000 * (i + 1)) for i in range(6)]
    for s in (float("inf"), float("-inf"), 65.0, -1e30):
        assert f(*P, 2, 5, 100, 77, 16, 320, 640, 640, 640, 640, 320, 1, C.c_float(0.125), C.c_float(s), None) == -1, s
