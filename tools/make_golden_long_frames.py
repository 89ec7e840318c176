#!/usr/bin/env python3
"""Generate the goldens of clips longer than 16 frames (17 <= T <= 32) by running the REAL reference modules on CPU: with
use_relative_position off the reference's TemporalTransformer.forward (attention.py:331-373) takes any frame count.

  block_long_frames.npz          tt24    TemporalTransformer(128 ch, 2 heads, linear, temporal_length 16), weights fill(., 31),
                                         x [1,128,24,3,5]
                                 ttc32   the causal one, temporal_length 32, weights fill(., 32), x [2,128,32,4,5]
                                         (sensitivity, asserted here: the same weights WITHOUT the mask give another output)
                                 rb24    ResBlock(64 -> 128, emb 256, TemporalConvBlock), weights fill(., 33), x [24,64,3,5], batch_size 1:
                                         the temporal conv and the 5-D GroupNorms over 24 frames on their own
  unet_reduced_long_frames.npz   the reduced-width UNet (tools/make_golden.py REDUCED, weights fill(., 11)):
                                 plain24   x [1,4,24,16,16]  uniform t, 77 tokens
                                 fifo32    x [1,4,32,8,40]   per-frame t (the reference's is_fifo branch), 77 tokens
                                 causal24  use_causal_attention, temporal_length 24   x [1,4,24,8,8]
  unet_reduced_long_frames_cross32.npz
                                 cross32   temporal_selfatt_only=False                x [1,4,32,32,64]  (h*w = 2048, 512, 128, 32)
                                 (a file of its own: every committed fixture stays under 1 MiB)
  unet_full_long_frames.npz, unet_full_long_frames_b.npz
                                 (--full) the YAML's UNet at [1,4,32,40,64], per-frame t, 77 tokens: the shape with the largest
                                 GroupNorm statistics groups a T <= 32 forward produces at 40 x 64 latents; frames 0 .. 15 of the
                                 output and the call metadata in the first file, frames 16 .. 31 in the second

    python tools/make_golden_long_frames.py [--full | --only-full]

Same recipe as tools/make_golden.py (whose helpers it imports): parameters and inputs are regenerated bit-identically from
moca_video_amd.weightgen by name, so a fixture holds only expected outputs and call metadata."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
from make_golden_temporal_variants import SENS, fifo_t, full_params, relerr, run_unet  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
from test_unet_gpu import TOL_BLOCK, TOL_UNET  # noqa: E402


def blocks(om, att):
    out = {}
    with torch.no_grad():
        mk = lambda causal, tl, seed: MG.fill(att.TemporalTransformer(128, 2, 64, depth=1, use_linear=True, use_checkpoint=False,
                                                                      only_self_att=True, causal_attention=causal,
                                                                      relative_position=False, temporal_length=tl).eval(), seed)
        out["tt24"] = mk(False, 16, 31)(MG.inp("lf.tt24.x", (1, 128, 24, 3, 5)))
        x = MG.inp("lf.ttc32.x", (2, 128, 32, 4, 5))
        out["ttc32"], y_plain = mk(True, 32, 32)(x), mk(False, 32, 32)(x)
        sens = relerr(y_plain, out["ttc32"])
        print(f"[block] ttc32: dropping the mask moves it by {sens:.3e} of max|y| (need > {SENS * TOL_BLOCK:.1e})")
        assert sens > SENS * TOL_BLOCK, "the causal mask is not visible in this fixture"
        rb = MG.fill(om.ResBlock(64, 256, 0.0, out_channels=128, dims=2, use_checkpoint=False, use_temporal_conv=True).eval(), 33)
        out["rb24"] = rb(MG.inp("lf.rb24.x", (24, 64, 3, 5)), MG.inp("lf.rb24.emb", (24, 256)), batch_size=1)
        for k, v in out.items():
            print(f"[block] {k}: {tuple(v.shape)} std {v.std():.4f}")
    MG.save("block_long_frames", **out)


def unets(om):
    out = {}
    mk = lambda **kw: MG.fill(om.UNetModel(**dict(MG.REDUCED, **kw)).eval(), 11)
    with torch.no_grad():
        plain = mk()
        out.update(run_unet(plain, "lf", "plain24", (1, 4, 24, 16, 16), [500], 77, [16]))
        out.update(run_unet(plain, "lf", "fifo32", (1, 4, 32, 8, 40), fifo_t(32), 77, [10]))
        causal = mk(use_causal_attention=True, temporal_length=24)
        out.update(run_unet(causal, "lf", "causal24", (1, 4, 24, 8, 8), [500], 77, [16]))
        y_plain = run_unet(plain, "lf", "causal24", (1, 4, 24, 8, 8), [500], 77, [16])["causal24"]
        sens = relerr(y_plain, out["causal24"])
        print(f"[lf] causal24: dropping the mask moves the output by {sens:.3e} of max|y| (need > {SENS * TOL_UNET:.1e})")
        assert sens > SENS * TOL_UNET, "the causal mask is not visible at the UNet output"
        MG.save("unet_reduced_long_frames", **out)
        cross = mk(temporal_selfatt_only=False)
        MG.save("unet_reduced_long_frames_cross32", **run_unet(cross, "lf", "cross32", (1, 4, 32, 32, 64), fifo_t(32), 77, [10]))


def full_case(om):
    t0 = time.time()
    model = MG.fill(om.UNetModel(**full_params()).eval(), 11)
    print(f"[full_long] reference UNet built+filled in {time.time() - t0:.1f}s")
    with torch.no_grad():
        out = run_unet(model, "full_long", "fifo32", (1, 4, 32, 40, 64), fifo_t(32), 77, [10], ctx_dim=1024)
    y = out.pop("fifo32")                      # 1.3 MB of float32: frames 0 .. 15 here, 16 .. 31 in a file of their own (1 MiB per file)
    MG.save("unet_full_long_frames", fifo32=y[:, :, :16], **out)
    MG.save("unet_full_long_frames_b", fifo32=y[:, :, 16:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--only-full", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(8)
    om, att = MG.import_reference()
    if not a.only_full:
        blocks(om, att)
        unets(om)
    if a.full or a.only_full:
        full_case(om)


if __name__ == "__main__":
    main()
