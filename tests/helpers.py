"""Shared test helpers: deterministic inputs (same recipe as tools/make_golden.py) and golden loading."""
import os

import numpy as np
import torch

from moca_video_amd.weightgen import gen_state_dict, gen_tensor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

REDUCED = dict(in_channels=4, out_channels=4, model_channels=64, attention_resolutions=[4, 2, 1], num_res_blocks=2,
               channel_mult=[1, 2, 4, 4], num_head_channels=64, transformer_depth=1, context_dim=128, use_linear=True,
               use_checkpoint=False, temporal_conv=True, temporal_attention=True, temporal_selfatt_only=True,
               use_relative_position=False, use_causal_attention=False, temporal_length=16, addition_attention=True,
               fps_cond=True)

FULL = dict(in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2,
            channel_mult=[1, 2, 4, 4], num_head_channels=64, transformer_depth=1, context_dim=1024, use_linear=True,
            use_checkpoint=True, temporal_conv=True, temporal_attention=True, temporal_selfatt_only=True,
            use_relative_position=False, use_causal_attention=False, temporal_length=16, addition_attention=True,
            fps_cond=True)


def inp(name, shape, seed=0):
    t = gen_tensor("input:" + name, (int(np.prod(shape)),), seed)
    return (t * 10.0).reshape(shape)


def golden(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


def golden_host_math():
    """`with golden_host_math():` -- the oracle's per-step float32 sqrt / exp return what the host that made the goldens computed
    (oracle/hostmath.py, tests/golden/host_math_f32.npz): torch's last bit differs between CPU vendors, and a bit-exact comparison
    with a golden must not depend on the host it runs on"""
    from oracle import hostmath
    g = golden("host_math_f32")
    return hostmath.pinned({k: (g[k + "_x"], g[k + "_y"]) for k in ("sqrt", "exp")})


def state_dict_for(module, seed):
    """weightgen parameters for a module built by OUR classes (same keys/shapes as the reference)."""
    return gen_state_dict({k: v.shape for k, v in module.state_dict().items()}, seed)


def relerr(got, ref):
    """max|got - ref| / max|ref|.  With MOCA_ERRLOG=<file> every value is appended with the running test's id (how the
    tolerances in the GPU tests were set: <= 1.5 x the largest value observed there)."""
    got = torch.as_tensor(got).float()
    ref = torch.as_tensor(ref).float()
    e = ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()
    log = os.environ.get("MOCA_ERRLOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{e:.3e} {os.environ.get('PYTEST_CURRENT_TEST', '?')}\n")
    return e


def loop_sam_candidates(call, F, H, W):
    """Scripted Grounded-SAM-2 output for the `call`-th `ddim_step` of a sampling loop, one entry per frame (None = no box
    detected): tools/make_golden.py::loop_cases feeds these to the REAL reference through fake predictor objects, the tests
    hand the same lists to the oracle / the HIP path as `sam_masks`.  Cycles through: a detection, a shifted detection (IoU
    fallback), no detection, a > 80 % mask followed by a small one, and an empty list."""
    def rect(y0, y1, x0, x1):
        m = torch.zeros(H, W)
        m[y0 % H:max(y0 % H + 1, y1 % (H + 1)), x0 % W:max(x0 % W + 1, x1 % (W + 1))] = 1.0
        return m
    big = torch.ones(H, W)
    out = []
    for i in range(F):
        k = (call * 3 + i) % 5
        if k == 0:
            out.append(rect(2 + call, 10 + call, 3, 12)[None])
        elif k == 1:
            out.append(rect(2 + call, 10 + call, 4 + i, 12 + i)[None])
        elif k == 2:
            out.append(None)
        elif k == 3:
            out.append(torch.stack([big, rect(1, 5 + i, 1 + call, 6 + call)]))
        else:
            out.append(rect(11, 15, call % 4, 5 + call % 4)[None])
    return out


def wgroup_cases():
    """per-row-group weights (a GroupNorm folded into proj_in) on the 320 -> 320 linear: (group rows, M, residual, MOCA_TUNE_GEMM_WS,
    epilogue flag).  Group rows: 4096 (64 x 64 latents, per frame), 16 x 1024 (32 x 32 latents, per video), 2560 / 640 (multiples of
    the 160-row tile), 512 = 160 x 3 + 32 (not); M = the multiple of the group rows at or just above 2^15 .. 2^18"""
    out = []
    for rows in (4096, 1024 * 16, 2560, 640, 160 * 3 + 32):
        for lg in (15, 16, 17, 18):
            M = -(-(1 << lg) // rows) * rows
            for res in (False, True):
                for knob in (0, 1, 2):
                    for flag in ("plain", "rowsum", "ln", "colsum"):
                        out.append((rows, M, res, knob, flag))
    return out
