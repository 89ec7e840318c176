"""CPU: the OpenCLIP image embedders (moca_video_amd.clip_vision): state-dict surface, the fp32 restatement (tests/clip_vision_ref.py)
against transformers' CLIP vision model, the preprocessing rules, the refusals, the argument checks of the new entry points and the
ISA of the new kernels."""
import ctypes as C
import os
import shutil
import sys

import pytest
import torch

import clip_vision_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(width=160, heads=2, layers=3)


def _v2(**kw):
    from moca_video_amd.clip_vision import FrozenOpenCLIPImageEmbedderV2
    return FrozenOpenCLIPImageEmbedderV2(**kw)


def _v1(**kw):
    from moca_video_amd.clip_vision import FrozenOpenCLIPImageEmbedder
    return FrozenOpenCLIPImageEmbedder(**kw)


def test_state_dict_surface_and_parameter_count():
    """open_clip ViT-H-14 after `del model.transformer`: 632 076 800 visual parameters (transformers' CLIPVisionModelWithProjection
    at the same config) + 51 723 265 of the text remnants"""
    with torch.device("meta"):
        m = _v2()
    sd = m.state_dict()
    vis = {k: v for k, v in sd.items() if k.startswith("model.visual.")}
    rest = {k: v for k, v in sd.items() if not k.startswith("model.visual.")}
    assert sum(v.numel() for v in sd.values()) == 683_800_065
    assert sum(v.numel() for v in vis.values()) == 632_076_800
    assert sorted(rest) == ["model.ln_final.bias", "model.ln_final.weight", "model.logit_scale", "model.positional_embedding",
                            "model.text_projection", "model.token_embedding.weight"]
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes["model.visual.conv1.weight"] == (1280, 3, 14, 14)
    assert shapes["model.visual.class_embedding"] == (1280,)
    assert shapes["model.visual.positional_embedding"] == (257, 1280)
    assert shapes["model.visual.proj"] == (1280, 1024)
    assert shapes["model.visual.ln_pre.weight"] == shapes["model.visual.ln_post.bias"] == (1280,)
    assert shapes["model.token_embedding.weight"] == (49408, 1024) and shapes["model.text_projection"] == (1024, 1024)
    assert shapes["model.positional_embedding"] == (77, 1024) and shapes["model.logit_scale"] == ()
    blk = {k[len("model.visual.transformer.resblocks.31."):]: v for k, v in shapes.items()
           if k.startswith("model.visual.transformer.resblocks.31.")}
    assert blk == {"ln_1.weight": (1280,), "ln_1.bias": (1280,), "attn.in_proj_weight": (3840, 1280), "attn.in_proj_bias": (3840,),
                   "attn.out_proj.weight": (1280, 1280), "attn.out_proj.bias": (1280,), "ln_2.weight": (1280,), "ln_2.bias": (1280,),
                   "mlp.c_fc.weight": (5120, 1280), "mlp.c_fc.bias": (5120,), "mlp.c_proj.weight": (1280, 5120), "mlp.c_proj.bias": (1280,)}
    assert not any(k.startswith("model.visual.transformer.resblocks.32.") for k in sd)
    with torch.device("meta"):
        assert set(_v1().state_dict()) == set(sd)


def test_strict_load_of_a_weightgen_state_dict():
    from helpers import state_dict_for
    for make in (_v1, _v2):
        m = make(**SMALL)
        sd = state_dict_for(m, 31)
        m.load_state_dict(sd, strict=True)
        wrapped = torch.nn.Module()                     # an `embedder.*` checkpoint slice, as LatentVisualDiffusion holds it
        wrapped.embedder = m
        wrapped.load_state_dict({"embedder." + k: v for k, v in sd.items()}, strict=True)
        assert not any(p.requires_grad for p in m.parameters())


def _hf_model(sd, width, heads, layers, output_dim):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPVisionConfig(hidden_size=width, intermediate_size=4 * width, num_attention_heads=heads, num_hidden_layers=layers,
                                        image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5, projection_dim=output_dim,
                                        attention_dropout=0.0)
    hf = transformers.CLIPVisionModelWithProjection(cfg).eval()
    g = lambda n: sd["model.visual." + n].float()
    w = {"vision_model.embeddings.patch_embedding.weight": g("conv1.weight"),
         "vision_model.embeddings.class_embedding": g("class_embedding"),
         "vision_model.embeddings.position_embedding.weight": g("positional_embedding"),
         "vision_model.pre_layrnorm.weight": g("ln_pre.weight"), "vision_model.pre_layrnorm.bias": g("ln_pre.bias"),
         "vision_model.post_layernorm.weight": g("ln_post.weight"), "vision_model.post_layernorm.bias": g("ln_post.bias"),
         "visual_projection.weight": g("proj").t()}
    for i in range(layers):
        r, h = f"transformer.resblocks.{i}.", f"vision_model.encoder.layers.{i}."
        for n, t in zip("qkv", g(r + "attn.in_proj_weight").split(width)):
            w[h + f"self_attn.{n}_proj.weight"] = t
        for n, t in zip("qkv", g(r + "attn.in_proj_bias").split(width)):
            w[h + f"self_attn.{n}_proj.bias"] = t
        for ours, theirs in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                             ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            w[h + theirs + ".weight"], w[h + theirs + ".bias"] = g(r + ours + ".weight"), g(r + ours + ".bias")
    missing, unexpected = hf.load_state_dict(w, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return hf


def test_restatement_matches_transformers_clip_vision_model():
    from helpers import inp, state_dict_for
    m = _v2(**SMALL)
    sd = state_dict_for(m, 31)
    hf = _hf_model(sd, 160, 2, 3, 1024)
    img = inp("clip_vision.cpu.img", (2, 3, 224, 224)).clamp(-1, 1)
    with torch.no_grad():
        out = hf(pixel_values=R.preprocess(img))
        v2, v1 = R.embed_v2(sd, img, 2), R.embed_v1(sd, img, 2)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    assert v2.shape == (2, 257, 160) and v1.shape == (2, 1024)
    assert rel(v2, out.last_hidden_state) < 2e-5
    assert rel(v1, out.image_embeds) < 2e-5


def test_preprocess_rules():
    from helpers import inp
    img = inp("clip_vision.cpu.pp", (1, 3, 224, 224)).clamp(-1, 1)
    ident = ((img + 1) / 2 - R.MEAN[:, None, None]) / R.STD[:, None, None]
    assert torch.allclose(R.preprocess(img), ident, atol=1e-6, rtol=0)          # 224 x 224: plain normalisation
    const = torch.full((1, 3, 320, 512), 0.25)
    out = R.preprocess(const)
    assert torch.allclose(out, out[:, :, :1, :1].expand_as(out), atol=1e-5, rtol=0)
    assert R.blur_params(320, 512)[0] == (3, 3)
    assert R.blur_params(1024, 1024)[0] == (7, 7)
    assert R.blur_params(160, 160) is None and R.blur_params(224, 224) is None  # upscale only / same size: no blur
    assert R.blur_params(320, 512, antialias=False) is None


def test_refusals():
    with pytest.raises(NotImplementedError):
        _v2(layer="penultimate")
    with pytest.raises(NotImplementedError):
        _v1(layer="penultimate", **SMALL)
    with pytest.raises(NotImplementedError):
        _v2(width=128, heads=2, layers=1)                # head dim 64
    with pytest.raises(NotImplementedError):
        _v2(arch="ViT-L-14")
    m = _v1(ucg_rate=0.1, **SMALL)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 224, 224))
    with pytest.raises((RuntimeError, ValueError)):      # no CPU path
        m(torch.zeros(1, 3, 224, 224), no_dropout=True)
    with pytest.raises((RuntimeError, ValueError)):
        _v2(**SMALL)(torch.zeros(1, 3, 224, 224))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from moca_video_amd import lib
    l = lib.load()
    p = C.c_void_p(4096)
    assert l.moca_attention_d80_f16(None, None, None, None, 1, 16, 257, 3840, 3840, 3840, 1280, 80 ** -0.5, None) == -1
    assert l.moca_attention_d80_f16(p, p, p, p, 1, 16, 0, 3840, 3840, 3840, 1280, 80 ** -0.5, None) == -1        # N = 0
    assert l.moca_attention_d80_f16(p, p, p, p, 1, 16, 257, 1000, 3840, 3840, 1280, 80 ** -0.5, None) == -1      # ldq < heads * 80
    assert l.moca_attention_d80_f16(p, p, p, p, 1, 16, 257, 3844, 3840, 3840, 1280, 80 ** -0.5, None) == -1      # ldq % 8
    assert l.moca_attention_d80_f16(C.c_void_p(4098), p, p, p, 1, 16, 257, 3840, 3840, 3840, 1280, 0.1, None) == -1  # misaligned q
    assert l.moca_attention_d80_f16(p, p, p, p, 1, 16, 257, 3840, 3840, 3840, 1280, float("inf"), None) == -1
    assert l.moca_attention_d80_f16(p, p, p, p, 1, 16, 257, 3840, 3840, 3840, 1280, float("nan"), None) == -1
    assert l.moca_clip_preprocess_patches_f16(None, 1, None, 1, 320, 512, 224, 14, 608, 1, None) == -1
    assert l.moca_clip_preprocess_patches_f16(p, 1, p, 1, 320, 512, 224, 14, 584, 1, None) == -1              # ldo < 588
    assert l.moca_clip_preprocess_patches_f16(p, 1, p, 1, 320, 512, 224, 14, 604, 1, None) == -1              # ldo % 8
    assert l.moca_clip_preprocess_patches_f16(p, 1, p, 1, 320, 512, 220, 14, 608, 1, None) == -1              # size % patch
    assert l.moca_clip_preprocess_patches_f16(p, 1, p, 1, 1, 512, 224, 14, 608, 1, None) == -1                # H < 2
    assert l.moca_clip_preprocess_patches_f16(p, 1, p, 1, 16384, 16384, 224, 14, 608, 1, None) == -1          # > 63 blur taps
    assert l.moca_clip_assemble_tokens_f16(None, 1280, None, None, None, 1, 256, 1280, None) == -1
    assert l.moca_clip_assemble_tokens_f16(p, 1000, p, p, p, 1, 256, 1280, None) == -1                         # ldp < C


def test_isa_of_the_new_kernels():
    """present in the library, no scratch / spills, and the attention kernel within the <= 128 registers (four waves per SIMD) its
    header comment (csrc/clip_vision.hip) claims"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from moca_video_amd import lib
    if not os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")) or shutil.which("c++filt") is None:
        pytest.skip("llvm-objdump / c++filt not available")
    r = isa_report.analyse(lib.LIB_PATH)
    # (kernels with _Float16 in their signature stay mangled: c++filt does not know DF16_)
    pick = lambda stem: [v for k, v in r.items() if stem in k]
    for stem in ("clip_attention_d80_kernel", "clip_preprocess_patches_kernelIf", "clip_preprocess_patches_kernelIDF16_",
                 "clip_assemble_tokens_kernel"):
        found = pick(stem)
        assert len(found) == 1, f"{stem}: {len(found)} kernels in the library"
        d = found[0]
        assert d["scratch"] == 0 and d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0, stem
    att = pick("clip_attention_d80_kernel")[0]
    assert att.get("vgpr_count", 0) + att.get("agpr_count", 0) <= 128
    assert att["mfma_total"] % 32 == 0           # per key tile: 4 sub-tiles x 3 k-steps (S^T) + 5 d-tiles x 4 sub-tiles (P.V); hipcc peels
