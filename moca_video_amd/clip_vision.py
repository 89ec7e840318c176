"""MI355X-native image embedder of the i2v model: the OpenCLIP ViT-H/14 vision tower behind `FrozenOpenCLIPImageEmbedderV2`
(`lvdm/modules/encoders/condition.py:298-376`, the token features the `Resampler` consumes) and `FrozenOpenCLIPImageEmbedder`
(`:238-296`, the pooled embedding `ImageProjModel` consumes).

Per image: `preprocess` (kornia's antialiased bicubic resize to 224 x 224, (x + 1) / 2, CLIP mean / std) and conv1's patchify in one
kernel (`moca_clip_preprocess_patches_f16`, writing the patch GEMM's A operand), conv1 as a GEMM with K = 588 padded to 608,
[class token; patches] + positional embedding (`moca_clip_assemble_tokens_f16`), `ln_pre`, then 32 pre-LN resblocks on the text
tower's kernels -- LayerNorm, the fused in_proj GEMM, head-dim-80 attention (`moca_attention_d80_f16`), out_proj + residual, c_fc with
the exact-GELU epilogue, c_proj + residual.  V1 adds `ln_post` on the class token and `@ proj`.  `patch_dropout` is the identity at
inference; only the conv1 patch path is built (`input_patchnorm` is for dual-patchnorm models, and ViT-H/14 has none).

Choices that cannot be checked offline (`open_clip_torch` and `kornia` are not installed, and the `laion2b_s32b_b79k` weights are
not available):
  * Attention is per image over its 257 tokens, as open_clip's own `visual()` and `transformers.CLIPVisionModel` compute it.  V2
    permutes NLD -> LND before `self.model.visual.transformer`; which layout that `Transformer` expects depends on the open_clip
    version (`batch_first`), so the reference's result at B > 1 may differ from this one; per-image attention is the tower's intent.
  * The state dict is what the reference module holds after `del model.transformer`: `model.visual.*` plus the text remnants
    `model.token_embedding`, `model.positional_embedding`, `model.ln_final`, `model.text_projection`, `model.logit_scale` (unused
    here).  That key list is taken from open_clip's source (`CLIP.__init__` / `VisionTransformer.__init__`), not from a live import.
  * The antialias rule is restated from kornia's `resize` (kornia/geometry/transform/affwarp.py): Gaussian pre-blur only when
    downscaling, sigma = max((factor - 1) / 2, 0.001) per axis, int(max(4 sigma, 3)) taps made odd, reflect border.  The reference
    pins kornia==0.5.6, and whether that version accepts `antialias=` at all is unverified; the torch restatement in
    tests/clip_vision_ref.py is what pins this behaviour.
There is no CPU path: forward raises on a CPU tensor.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .clip_text import _ResBlock
from .unet import _Param

__all__ = ["FrozenOpenCLIPImageEmbedderV2", "FrozenOpenCLIPImageEmbedder"]


class _VisionTransformer(nn.Module):
    """open_clip VisionTransformer parameters (conv1 without bias, class / positional embedding, ln_pre, resblocks, ln_post, proj)"""

    def __init__(self, width, layers, patch, image, output_dim):
        super().__init__()
        grid = image // patch
        self.conv1 = _Param((width, 3, patch, patch), bias=False)
        self.class_embedding = nn.Parameter(torch.empty(width), requires_grad=False)
        self.positional_embedding = nn.Parameter(torch.empty(grid * grid + 1, width), requires_grad=False)
        self.ln_pre = _Param((width,), kind="norm")
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.ModuleList([_ResBlock(width) for _ in range(layers)])
        self.ln_post = _Param((width,), kind="norm")
        self.proj = nn.Parameter(torch.empty(width, output_dim), requires_grad=False)


class _CLIPRemnant(nn.Module):
    """open_clip CLIP after `del model.transformer`: the vision tower and the text tower's remaining parameters (ViT-H-14 text config)"""

    def __init__(self, width, layers, patch, image, output_dim, vocab=49408, context=77, text_width=1024):
        super().__init__()
        self.visual = _VisionTransformer(width, layers, patch, image, output_dim)
        self.token_embedding = _Param((vocab, text_width), bias=False)
        self.positional_embedding = nn.Parameter(torch.empty(context, text_width), requires_grad=False)
        self.ln_final = _Param((text_width,), kind="norm")
        self.text_projection = nn.Parameter(torch.empty(text_width, output_dim), requires_grad=False)
        self.logit_scale = nn.Parameter(torch.empty(()), requires_grad=False)


class _OpenCLIPVision(nn.Module):
    def __init__(self, arch, version, device, freeze, layer, antialias, width, heads, layers, patch, image, output_dim):
        super().__init__()
        if layer == "penultimate":
            raise NotImplementedError("layer='penultimate' (the reference raises too)")
        if arch != "ViT-H-14" and (width, heads, layers, patch, image, output_dim) == (1280, 16, 32, 14, 224, 1024):
            raise NotImplementedError(f"arch {arch!r}: pass width/heads/layers/patch/image/output_dim explicitly (only the ViT-H-14 "
                                      "vision tower is built in)")
        if width % heads or width // heads != 80:
            raise NotImplementedError("the vision attention kernel is head-dim 80")
        if image % patch:
            raise ValueError(f"image size {image} is not a multiple of the patch size {patch}")
        self.model = _CLIPRemnant(width, layers, patch, image, output_dim)
        self.device = device
        self.layer, self.antialias = layer, antialias
        self.width, self.heads, self.patch, self.image, self.output_dim = width, heads, patch, image, output_dim
        self.register_buffer("mean", torch.tensor([0.48145466, 0.4578275, 0.40821073]), persistent=False)
        self.register_buffer("std", torch.tensor([0.26862954, 0.26130258, 0.27577711]), persistent=False)
        if freeze:
            self.freeze()
        self._packed = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_packed", None))

    def freeze(self):
        self.model = self.model.eval()
        for p in self.model.parameters():
            p.requires_grad = False

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._packed = None
        return out

    def _pack(self):
        vis = self.model.visual
        dev = vis.positional_embedding.device
        if dev.type != "cuda":
            raise RuntimeError(f"moca_video_amd.{type(self).__name__} runs on an MI355X only; call .cuda() first (no CPU path)")
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        k = 3 * self.patch * self.patch
        w1 = torch.zeros(self.width, ops._round_up(k, 32), dtype=torch.float32)   # K padded to a multiple of 32 with zero columns
        w1[:, :k] = vis.conv1.weight.detach().float().reshape(self.width, k).cpu()
        P = {"conv1": ops.pack_linear(w1, None, device=dev), "cls": f32(vis.class_embedding), "pos": f32(vis.positional_embedding),
             "ln_pre": (f32(vis.ln_pre.weight), f32(vis.ln_pre.bias)), "ln_post": (f32(vis.ln_post.weight), f32(vis.ln_post.bias)),
             "proj": ops.pack_linear(vis.proj.detach().t(), None, device=dev), "blocks": []}
        for r in vis.transformer.resblocks:
            P["blocks"].append(dict(
                ln1=(f32(r.ln_1.weight), f32(r.ln_1.bias)), ln2=(f32(r.ln_2.weight), f32(r.ln_2.bias)),
                qkv=ops.pack_linear(r.attn.in_proj_weight.detach(), r.attn.in_proj_bias.detach(), device=dev),
                out=ops.pack_linear(r.attn.out_proj.weight.detach(), r.attn.out_proj.bias.detach(), device=dev),
                fc=ops.pack_linear(r.mlp.c_fc.weight.detach(), r.mlp.c_fc.bias.detach(), device=dev),
                proj=ops.pack_linear(r.mlp.c_proj.weight.detach(), r.mlp.c_proj.bias.detach(), device=dev)))
        self._packed = P

    @torch.no_grad()
    def _tower(self, image):
        """image [B, 3, H, W] in [-1, 1] -> (residual stream after the last resblock, fp16 [B * 257][>= width] (columns past width are
        the GEMMs' zero padding), B)"""
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"expected images [B, 3, H, W], got {tuple(image.shape)}")
        if not image.is_cuda:
            raise ValueError(f"moca_video_amd.{type(self).__name__} needs CUDA (HIP) images; there is no CPU path")
        if self._packed is None:
            self._pack()
        if image.dtype not in (torch.float32, torch.float16):
            image = image.float()
        image = image.contiguous()
        P, C, H = self._packed, self.width, self.heads
        B, G = image.shape[0], self.image // self.patch
        T = G * G + 1
        M, dev = B * T, image.device
        ops.set_stream(None)
        new = lambda rows, pw, dt=torch.float16: torch.empty(rows, pw.N, dtype=dt, device=dev)   # GEMM outputs: pw.N = N padded to 64

        def rows(t, n):                          # [M][n] contiguous operand of the LayerNorm / attention kernels
            return t if t.shape[1] == n else t[:, :n].contiguous()
        a = torch.empty(B * (T - 1), P["conv1"].K, dtype=torch.float16, device=dev)
        ops.clip_preprocess_patches(image, a, size=self.image, patch=self.patch, antialias=self.antialias)
        pe = ops.gemm(a, P["conv1"], new(B * (T - 1), P["conv1"], torch.float32), M=B * (T - 1), out_f32=True)
        x = ops.clip_assemble_tokens(pe, P["cls"], P["pos"], torch.empty(M, C, dtype=torch.float16, device=dev), B=B, P=T - 1, Cn=C)
        x = ops.layernorm(x, torch.empty_like(x), *P["ln_pre"], M=M, Cn=C)
        if C % 64:                               # the residual stream takes the row stride of the GEMMs that write it (N padded to 64)
            xp = torch.zeros(M, ops._round_up(C, 64), dtype=torch.float16, device=dev)
            xp[:, :C] = x
            x = xp
        for blk in P["blocks"]:
            l = ops.layernorm(rows(x, C), torch.empty(M, C, dtype=torch.float16, device=dev), *blk["ln1"], M=M, Cn=C)
            qkv = ops.gemm(l, blk["qkv"], new(M, blk["qkv"]), M=M)
            ld = qkv.stride(0)
            att = ops.attention_d80(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], torch.empty(M, C, dtype=torch.float16, device=dev),
                                    B=B, heads=H, N=T, ldq=ld, ldk=ld, ldv=ld, ldo=C, scale=80 ** -0.5)
            x = ops.gemm(att, blk["out"], new(M, blk["out"]), M=M, residual=x)
            l = ops.layernorm(rows(x, C), torch.empty(M, C, dtype=torch.float16, device=dev), *blk["ln2"], M=M, Cn=C)
            h = ops.gemm(l, blk["fc"], new(M, blk["fc"]), M=M, gelu=True)
            x = ops.gemm(h, blk["proj"], new(M, blk["proj"]), M=M, residual=x)
        return x, B

    def encode(self, image):
        return self(image)


class FrozenOpenCLIPImageEmbedderV2(_OpenCLIPVision):
    """condition.py:298-376.  forward(image [B, 3, H, W], values in [-1, 1], fp32 or fp16) -> fp32 [B, 257, 1280]: the transformer
    output BEFORE `ln_post` (what `Resampler` consumes)."""

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", freeze=True, layer="pooled", antialias=True,
                 width=1280, heads=16, layers=32, patch=14, image=224, output_dim=1024):
        super().__init__(arch, version, device, freeze, layer, antialias, width, heads, layers, patch, image, output_dim)

    def forward(self, image, no_dropout=False):
        return self.encode_with_vision_transformer(image)

    def encode_with_vision_transformer(self, image):
        x, B = self._tower(image)
        return x[:, :self.width].float().reshape(B, -1, self.width)


class FrozenOpenCLIPImageEmbedder(_OpenCLIPVision):
    """condition.py:238-296.  forward(image [B, 3, H, W], values in [-1, 1], fp32 or fp16) -> fp32 [B, 1024]: `visual()` in full,
    `ln_post` on the class token and `@ proj` (what `ImageProjModel` consumes).  The reference runs this under `autocast` and so
    returns fp16; this one returns fp32.  `ucg_rate > 0` (training-time conditioning dropout) is refused in a forward without
    `no_dropout=True`."""

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True, layer="pooled",
                 antialias=True, ucg_rate=0., width=1280, heads=16, layers=32, patch=14, image=224, output_dim=1024):
        super().__init__(arch, version, device, freeze, layer, antialias, width, heads, layers, patch, image, output_dim)
        self.max_length = max_length
        self.ucg_rate = ucg_rate

    def forward(self, image, no_dropout=False):
        if self.ucg_rate > 0. and not no_dropout:
            raise NotImplementedError("ucg_rate > 0: the training-time conditioning dropout is not implemented (pass no_dropout=True)")
        return self.encode_with_vision_transformer(image)

    @torch.no_grad()
    def encode_with_vision_transformer(self, image):
        x, B = self._tower(image)
        P, C = self._packed, self.width
        cls = x.reshape(B, -1, x.shape[1])[:, 0, :C].contiguous()
        cls = ops.layernorm(cls, torch.empty_like(cls), *P["ln_post"], M=B, Cn=C)
        out = ops.gemm(cls, P["proj"], torch.empty(B, P["proj"].N, dtype=torch.float32, device=x.device), M=B, out_f32=True)
        return out[:, :self.output_dim].contiguous()
