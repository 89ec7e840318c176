"""Host-generated operands and the fp32 torch restatement of attention.py:92-114 (mask: :101-105) for the tests of temporal attention
over 17 .. 32 frames (tests/test_long_frames_gpu.py).  Operands come from moca_video_amd.weightgen (numpy Philox keyed by name): the
same bits in every process, on every host."""
import numpy as np
import torch

from moca_video_amd.weightgen import gen_tensor
from temporal_variants_ref import SCALE, attention_ref  # noqa: F401  (one restatement of the reference's attention for both files)

# B, T, HW, heads: one frame past the old limit with a grid tail (3 problems, 4 per block); the batch stride with odd HW; the last key
# and query row masked; a full tile with the production head count
KERNEL = [(1, 17, 3, 1), (2, 24, 21, 3), (1, 31, 5, 2), (1, 32, 64, 5)]
STRIDED = (2, 24, 7, 2)        # ld_qkv = 3C + 8, ldo = C + 4, q / k / v views of one buffer at non-zero column offsets


def host(name, *shape, scale=1.0):
    n = int(np.prod(shape))
    return (gen_tensor("input:lf." + name, (n,)) * 10.0 * scale).reshape(shape)


def operands(B, T, HW, heads, tag="k"):
    """fp16 [B*T*HW][3C] on the GPU: q | k | v"""
    C = heads * 64
    return host(f"{tag}.{B}.{T}.{HW}.{heads}", B * T * HW, 3 * C).half().cuda()


def reference(q, k, v, B, T, HW, heads, causal):
    """q, k, v: [B*T*HW][>= C] views (any row stride); returns fp32 [B*T*HW][C]"""
    C = heads * 64
    x = [t[:, :C].float().reshape(B, T, HW, heads, 64).permute(0, 2, 3, 1, 4) for t in (q, k, v)]      # [B, HW, heads, T, 64]
    return attention_ref(x[0], x[1], x[2], causal).permute(0, 3, 1, 2, 4).reshape(B * T * HW, C)
