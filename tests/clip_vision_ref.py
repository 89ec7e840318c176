"""fp32 torch restatement of the OpenCLIP image embedders (condition.py:238-376 + open_clip's VisionTransformer) for the tests of
moca_video_amd.clip_vision: preprocess (kornia resize with antialias, (x + 1) / 2, CLIP mean / std), the vision tower, V2's token
features before ln_post and V1's pooled projection.  Takes the module's state dict (keys `model.visual.*`).

kornia is not installed, so `preprocess` restates kornia.geometry.resize(x, (224, 224), interpolation="bicubic", align_corners=True,
antialias=True) from its source (kornia/geometry/transform/affwarp.py): when max(H / 224, W / 224) > 1, gaussian_blur2d with
sigma = max((factor - 1) / 2, 0.001) per axis, kernel size int(max(2 * 2 * sigma, 3)) made odd, normalised taps exp(-x^2 / (2
sigma^2)) at x = i - size // 2, border "reflect"; then F.interpolate(mode="bicubic", align_corners=True)."""
import torch
import torch.nn.functional as F

MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073])
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711])


def blur_params(H, W, size=224, antialias=True):
    """((ky, kx), (sigma_y, sigma_x)) of the antialias pre-blur, or None when kornia skips it (no downscaling)"""
    fy, fx = H / size, W / size
    if not antialias or max(fy, fx) <= 1:
        return None
    sig = (max((fy - 1.0) / 2.0, 0.001), max((fx - 1.0) / 2.0, 0.001))
    ks = [int(max(2.0 * 2 * s, 3)) for s in sig]
    ks = tuple(k + 1 if k % 2 == 0 else k for k in ks)
    return ks, sig


def gaussian_taps(n, sigma):
    x = torch.arange(n, dtype=torch.float32) - n // 2
    g = torch.exp(-x.pow(2.0) / float(2 * sigma ** 2))
    return g / g.sum()


def preprocess(img, size=224, antialias=True):
    """img [B, 3, H, W] in [-1, 1] -> [B, 3, size, size] fp32, normalised"""
    x = img.float()
    bp = blur_params(x.shape[-2], x.shape[-1], size, antialias)
    if bp is not None:
        (ky, kx), (sy, sx) = bp
        k2 = gaussian_taps(ky, sy)[:, None] * gaussian_taps(kx, sx)[None, :]
        x = F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect")
        x = F.conv2d(x, k2.to(x.device).expand(3, 1, ky, kx), groups=3)
    x = F.interpolate(x, size=(size, size), mode="bicubic", align_corners=True)
    x = (x + 1.0) / 2.0
    return (x - MEAN.to(x.device)[:, None, None]) / STD.to(x.device)[:, None, None]


def patchify(x, patch, kp):
    """[B, 3, S, S] -> conv1's im2col rows [B * (S / patch)^2, kp], columns (c, ky, kx), zero from 3 * patch^2"""
    B, C, S, _ = x.shape
    g = S // patch
    p = x.reshape(B, C, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * patch * patch)
    return F.pad(p, (0, kp - p.shape[1]))


def _get(sd, name):
    return sd["model.visual." + name].float()       # (on the device the state dict lives on; the image goes there too)


def tower(sd, img, heads, size=224, antialias=True):
    """the transformer output before ln_post, [B, T, width] fp32 (per-image attention)"""
    w1 = _get(sd, "conv1.weight")
    width, patch = w1.shape[0], w1.shape[-1]
    x = F.conv2d(preprocess(img, size, antialias), w1, stride=patch)
    x = x.reshape(x.shape[0], width, -1).permute(0, 2, 1)
    cls = _get(sd, "class_embedding").expand(x.shape[0], 1, width)
    x = torch.cat([cls, x], 1) + _get(sd, "positional_embedding")
    ln = lambda t, n: F.layer_norm(t, (width,), _get(sd, n + ".weight"), _get(sd, n + ".bias"), 1e-5)
    x = ln(x, "ln_pre")
    B, T, dh = x.shape[0], x.shape[1], width // heads
    i = 0
    while f"model.visual.transformer.resblocks.{i}.ln_1.weight" in sd:
        r = f"transformer.resblocks.{i}."
        qkv = ln(x, r + "ln_1") @ _get(sd, r + "attn.in_proj_weight").t() + _get(sd, r + "attn.in_proj_bias")
        q, k, v = (t.reshape(B, T, heads, dh).transpose(1, 2) for t in qkv.split(width, -1))
        a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1) @ v
        a = a.transpose(1, 2).reshape(B, T, width)
        x = x + a @ _get(sd, r + "attn.out_proj.weight").t() + _get(sd, r + "attn.out_proj.bias")
        h = F.gelu(ln(x, r + "ln_2") @ _get(sd, r + "mlp.c_fc.weight").t() + _get(sd, r + "mlp.c_fc.bias"))
        x = x + h @ _get(sd, r + "mlp.c_proj.weight").t() + _get(sd, r + "mlp.c_proj.bias")
        i += 1
    return x


def embed_v2(sd, img, heads, **kw):
    """FrozenOpenCLIPImageEmbedderV2.forward: [B, T, width]"""
    return tower(sd, img, heads, **kw)


def embed_v1(sd, img, heads, **kw):
    """FrozenOpenCLIPImageEmbedder.forward: ln_post(class token) @ proj, [B, output_dim]"""
    x = tower(sd, img, heads, **kw)[:, 0]
    x = F.layer_norm(x, (x.shape[-1],), _get(sd, "ln_post.weight"), _get(sd, "ln_post.bias"), 1e-5)
    return x @ _get(sd, "proj")
