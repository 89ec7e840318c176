"""Host-generated operands and fp32 torch restatements for the temporal-attention kernel tests (tests/test_temporal_variants_gpu.py).
Operands come from moca_video_amd.weightgen (numpy Philox keyed by name): the same bits on every host, so the outputs of the
NON-causal entries can be pinned by hash against the parent commit (tests/golden/temporal_attention_parent_sha.npz)."""
import hashlib

import numpy as np
import torch

from moca_video_amd.weightgen import gen_tensor

STANDALONE = [(2, 16, 50, 5), (1, 8, 64, 8), (1, 16, 2560, 5), (3, 5, 7, 2)]                      # B, T, HW, heads (test_kernels_gpu.py:524)
FUSED = [(2, 640, 5, 320, False), (1, 1280, 5, 320, True), (2, 100, 8, 512, True), (1, 40, 20, 1280, False)]   # B, HW, heads, K, fold (:1119)
SCALE = 0.125


def host(name, *shape, scale=1.0):
    n = int(np.prod(shape))
    return (gen_tensor("input:tv." + name, (n,)) * 10.0 * scale).reshape(shape)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def standalone_operands(B, T, HW, heads):
    C = heads * 64
    return host(f"sa.{B}.{T}.{HW}.{heads}", B * T * HW, 3 * C).half().cuda()


def attention_ref(q, k, v, causal):
    """q, k, v fp32 [..., T, 64]: softmax(q k^T * SCALE [masked as attention.py:101-105]) v"""
    s = torch.einsum("...id,...jd->...ij", q, k) * SCALE
    if causal:
        T = s.shape[-1]
        mask = torch.tril(torch.ones(T, T, device=s.device))                   # attention.py:311
        s = s.masked_fill(~(mask > 0.5), -torch.finfo(s.dtype).max)
    return torch.einsum("...ij,...jd->...id", s.softmax(-1), v)


def standalone_ref(qkv, B, T, HW, heads, causal):
    C = heads * 64
    x = qkv.float().view(B, T, HW, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)      # [3, B, HW, heads, T, 64]
    return attention_ref(x[0], x[1], x[2], causal).permute(0, 3, 1, 2, 4).reshape(B * T * HW, C)


def fused_operands(B, HW, heads, K, fold):
    """x, (wq, wk, wv), (gamma, beta) or None -- as test_gemm_temporal_attention_fused builds them"""
    C, M = heads * 64, B * 16 * HW
    tag = f"fu.{B}.{HW}.{heads}.{K}.{int(fold)}"
    x = (host(tag + ".x", M, K) * 1.5 + (0.3 if fold else 0.0)).half().cuda()
    ws = tuple(host(f"{tag}.w{i}", C, K, scale=K ** -0.5).half().cuda() for i in range(3))
    gb = None
    if fold:
        gb = ((host(tag + ".g", K) * 0.3 + 1.0).cuda(), (host(tag + ".b", K) * 0.3).cuda())
    return x, ws, gb


def fused_run(ops, x, ws, gb, B, HW, heads, causal):
    """one MOCA_EP_TATTN launch; returns the fp16 output [M][C]"""
    import torch.nn.functional as F
    C, M, K = heads * 64, x.shape[0], x.shape[1]
    kw = {}
    if gb is not None:
        wf, bf = ops.fold_layernorm(torch.cat(ws), None, gb[0], gb[1])
        pw = ops.finish_lnfold(ops.pack_qkv_per_head(wf[:C], wf[C:2 * C], wf[2 * C:], heads, bias=bf))
        xf = x.float()
        kw = dict(lnfold=(torch.stack([xf.sum(1), (xf * xf).sum(1)], dim=1).contiguous(), 1, 1e-5))
    else:
        pw = ops.pack_qkv_per_head(*ws, heads)
    tattn = (16, HW, SCALE, True) if causal else (16, HW, SCALE)
    assert ops.gemm_tattn_ok(x, pw, M=M, tattn=tattn, **({"lnfold": (None, 1, 1e-5)} if gb is not None else {}))
    out = torch.full((M, C), float("nan"), dtype=torch.float16, device=x.device)
    ops.gemm(x, pw, out, M=M, tattn=tattn, **kw)
    return out


def fused_ref(x, ws, gb, B, HW, heads, causal):
    """projection (rounded to fp16, as the two-launch path stores it) + attention over the frames in fp32 torch"""
    import torch.nn.functional as F
    C, M, K = heads * 64, x.shape[0], x.shape[1]
    a = x.float() if gb is None else F.layer_norm(x.float(), (K,), gb[0], gb[1], 1e-5)
    q, k, v = ((a @ w.float().t()).half().float().view(B, 16, HW, heads, 64).permute(0, 2, 3, 1, 4) for w in ws)   # [B, HW, h, T, 64]
    return attention_ref(q, k, v, causal).permute(0, 3, 1, 2, 4).reshape(M, C)
