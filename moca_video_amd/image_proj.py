"""MI355X-native image projectors of `LatentVisualDiffusion` (`lvdm/modules/encoders/ip_resampler.py`; chosen by `init_projector`,
ddpm3d.py:664-687): `ImageProjModel` (finegrained=False: 4 tokens from a [B, 1024] image embedding) and `Resampler` (finegrained=True:
16 tokens from [B, 257, 1280] image-token features).  They run once per video, so nothing here is tuned; every op is an existing
kernel of the library: the linears are `moca_gemm_f16` (exact-GELU epilogue `MOCA_EP_GELU` for the feed-forward, residual epilogue for
the two residual adds), the norms `moca_layernorm_f16`, the Perceiver attention `moca_attention_f16` with 16 queries over the 257 + 16
keys of `cat(x, latents)` (ip_resampler.py:71-72): the two LayerNorm outputs are written into adjacent rows of one buffer so that
`to_kv` is one GEMM.  Parameter names are the reference's, so a `image_proj_model.*` checkpoint loads unchanged.
Activations are fp16 (fp32 accumulate), the result is returned as fp32 like the reference's fp32 module."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import lib as _l
from . import ops
from .unet import _Param

__all__ = ["ImageProjModel", "Resampler"]


def _f32(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class _Projector(nn.Module):
    def __init__(self):
        super().__init__()
        self._packed = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_packed", None))
        _l.load()

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._packed = None
        return out

    def _device(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"moca_video_amd.{type(self).__name__} runs on an MI355X only; call .cuda() first (no CPU path)")
        return dev

    def _input(self, x, shape_tail):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise ValueError(f"{type(self).__name__}: the features must be a CUDA (HIP) tensor")
        if tuple(x.shape[1:]) != tuple(shape_tail):
            raise ValueError(f"{type(self).__name__}: expected features [B, {', '.join(map(str, shape_tail))}], got {tuple(x.shape)}")
        return x.to(torch.float16).contiguous()


class ImageProjModel(_Projector):
    """ip_resampler.py:7-21: LayerNorm(proj(embeds)) as `clip_extra_context_tokens` tokens"""

    def __init__(self, cross_attention_dim=1024, clip_embeddings_dim=1024, clip_extra_context_tokens=4):
        super().__init__()
        self.cross_attention_dim = cross_attention_dim
        self.clip_embeddings_dim = clip_embeddings_dim
        self.clip_extra_context_tokens = clip_extra_context_tokens
        self.proj = _Param((clip_extra_context_tokens * cross_attention_dim, clip_embeddings_dim))
        self.norm = _Param((cross_attention_dim,), kind="norm")

    @torch.no_grad()
    def forward(self, image_embeds):
        dev = self._device()
        if self._packed is None:
            self._packed = dict(proj=ops.pack_linear(self.proj.weight, self.proj.bias, device=dev),
                                norm=(_f32(self.norm.weight, dev), _f32(self.norm.bias, dev)))
        P = self._packed
        x = self._input(image_embeds, (self.clip_embeddings_dim,))
        B, n, C = x.shape[0], self.clip_extra_context_tokens, self.cross_attention_dim
        ops.set_stream(None)
        t = ops.gemm(x, P["proj"], torch.empty(B, n * C, dtype=torch.float16, device=dev), M=B)
        y = ops.layernorm(t.view(B * n, C), torch.empty(B * n, C, dtype=torch.float16, device=dev), *P["norm"], M=B * n, Cn=C)
        return y.view(B, n, C).float()


class _PerceiverAttention(nn.Module):
    """ip_resampler.py:45-92 (parameter holders)"""

    def __init__(self, dim, dim_head, heads):
        super().__init__()
        inner = dim_head * heads
        self.dim_head, self.heads = dim_head, heads
        self.norm1 = _Param((dim,), kind="norm")
        self.norm2 = _Param((dim,), kind="norm")
        self.to_q = _Param((inner, dim), bias=False)
        self.to_kv = _Param((2 * inner, dim), bias=False)
        self.to_out = _Param((dim, inner), bias=False)


def _feed_forward(dim, mult):
    """ip_resampler.py:24-31: LayerNorm, Linear (no bias), GELU, Linear (no bias) -> names .0, .1, .3"""
    inner = int(dim * mult)
    return nn.Sequential(_Param((dim,), kind="norm"), _Param((inner, dim), bias=False), nn.Identity(), _Param((dim, inner), bias=False))


class Resampler(_Projector):
    """ip_resampler.py:95-140 (the Perceiver resampler of `finegrained=True`)"""

    def __init__(self, dim=1024, depth=8, dim_head=64, heads=16, num_queries=8, embedding_dim=768, output_dim=1024, ff_mult=4):
        super().__init__()
        if dim_head != 64:
            raise NotImplementedError("the attention kernel is head-dim 64")
        self.dim, self.heads, self.num_queries, self.embedding_dim, self.output_dim = dim, heads, num_queries, embedding_dim, output_dim
        self.latents = nn.Parameter(torch.empty(1, num_queries, dim), requires_grad=False)
        self.proj_in = _Param((dim, embedding_dim))
        self.proj_out = _Param((output_dim, dim))
        self.norm_out = _Param((output_dim,), kind="norm")
        self.layers = nn.ModuleList([nn.ModuleList([_PerceiverAttention(dim, dim_head, heads), _feed_forward(dim, ff_mult)])
                                     for _ in range(depth)])

    def _pack(self, dev):
        lin = lambda m: ops.pack_linear(m.weight, m.bias, device=dev)
        norm = lambda m: (_f32(m.weight, dev), _f32(m.bias, dev))
        P = dict(latents=self.latents.detach().to(device=dev, dtype=torch.float16).reshape(self.num_queries, self.dim).contiguous(),
                 proj_in=lin(self.proj_in), proj_out=lin(self.proj_out), norm_out=norm(self.norm_out), layers=[])
        for attn, ff in self.layers:
            P["layers"].append(dict(norm1=norm(attn.norm1), norm2=norm(attn.norm2), to_q=lin(attn.to_q), to_kv=lin(attn.to_kv),
                                    to_out=lin(attn.to_out), ff_norm=norm(ff[0]), ff1=lin(ff[1]), ff2=lin(ff[3])))
        self._packed = P

    @torch.no_grad()
    def forward(self, x):
        """x: image-token features [B, N, embedding_dim] (N = 257 for the ViT-H/14 tower) -> [B, num_queries, output_dim] fp32"""
        dev = self._device()
        if self._packed is None:
            self._pack(dev)
        P = self._packed
        if x.dim() != 3:
            raise ValueError(f"Resampler: expected features [B, N, {self.embedding_dim}], got {tuple(x.shape)}")
        B, N = x.shape[0], x.shape[1]
        x = self._input(x, (N, self.embedding_dim))
        D, nq, H = self.dim, self.num_queries, self.heads
        inner = 64 * H
        L = N + nq                                               # keys of cat(x, latents) per video
        new = lambda rows, cols: torch.empty(rows, cols, dtype=torch.float16, device=dev)
        ops.set_stream(None)
        xp = ops.gemm(x.view(B * N, -1), P["proj_in"], new(B * N, D), M=B * N)
        lat = new(B * nq, D)
        for b in range(B):                                       # latents.repeat(B, 1, 1)
            lat[b * nq:(b + 1) * nq].copy_(P["latents"])
        kv_in = new(B * L, D)                                    # per video: [LN1(x) rows | LN2(latents) rows]
        for lp in P["layers"]:
            for b in range(B):
                ops.layernorm(xp[b * N:(b + 1) * N], kv_in[b * L:b * L + N], *lp["norm1"], M=N, Cn=D)
                ops.layernorm(lat[b * nq:(b + 1) * nq], kv_in[b * L + N:(b + 1) * L], *lp["norm2"], M=nq, Cn=D)
            q = new(B * nq, inner)
            for b in range(B):
                ops.gemm(kv_in[b * L + N:(b + 1) * L], lp["to_q"], q[b * nq:(b + 1) * nq], M=nq)
            kv = ops.gemm(kv_in, lp["to_kv"], new(B * L, 2 * inner), M=B * L)
            a = ops.attention(q, kv[:, :inner], kv[:, inner:], new(B * nq, inner), Bq=B, heads=H, Nq=nq, Nk=L, ldq=inner, ldk=2 * inner,
                              ldv=2 * inner, ldo=inner, kv_div=1, scale=64 ** -0.5)       # (q d^-1/4)(k d^-1/4)^T, ip_resampler.py:77-80
            lat = ops.gemm(a, lp["to_out"], new(B * nq, D), M=B * nq, residual=lat)
            h = ops.layernorm(lat, new(B * nq, D), *lp["ff_norm"], M=B * nq, Cn=D)
            h = ops.gemm(h, lp["ff1"], new(B * nq, lp["ff1"].N), M=B * nq, gelu=True)
            lat = ops.gemm(h, lp["ff2"], new(B * nq, D), M=B * nq, residual=lat)
        y = ops.gemm(lat, P["proj_out"], new(B * nq, self.output_dim), M=B * nq)
        y = ops.layernorm(y, new(B * nq, self.output_dim), *P["norm_out"], M=B * nq, Cn=self.output_dim)
        return y.view(B, nq, self.output_dim).float()
