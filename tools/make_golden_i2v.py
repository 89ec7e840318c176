#!/usr/bin/env python3
"""Generate the image-conditioning goldens by running the REAL reference modules on CPU:

  unet_reduced_i2v.npz  the reference UNet built with `use_image_attention=True` (the image cross-attention of attention.py:59-64,
                        82-87,117-124 in every SpatialTransformer's attn2) at the reduced width of tools/make_golden.py;
  unet_full_i2v.npz     the same at full width (the YAML's params + use_image_attention) on [1, 4, 16, 40, 64] with 93 tokens (--full);
  image_proj.npz        `Resampler(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=1024)` and
                        `ImageProjModel(4 tokens, 1024 -> 1024)` of `init_projector` (ddpm3d.py:664-687) on seeded features, and both on
                        the stand-in embedder's features of a ZERO image (tests/i2v_standin.py): the unconditional image tokens that
                        `base_ddim_sampling` appends (funcs.py:207-210).

    python tools/make_golden_i2v.py [--full]

Same recipe as tools/make_golden.py (whose helpers it imports): parameters and inputs are regenerated bit-identically from
moca_video_amd.weightgen by name, so a fixture holds only the expected outputs and the call metadata."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
REDUCED_I2V = dict(MG.REDUCED, use_image_attention=True)


def projectors():
    from lvdm.modules.encoders.ip_resampler import ImageProjModel, Resampler
    from i2v_standin import StandInImageEmbedder
    res = MG.fill(Resampler(dim=1024, depth=4, dim_head=64, heads=12, num_queries=16, embedding_dim=1280, output_dim=1024,
                            ff_mult=4).eval(), 21)
    imp = MG.fill(ImageProjModel(clip_extra_context_tokens=4, cross_attention_dim=1024, clip_embeddings_dim=1024).eval(), 22)
    zero = torch.zeros(2, 3, 224, 224)
    with torch.no_grad():
        MG.save("image_proj",
                resampler=res(MG.inp("i2v.resampler.x", (2, 257, 1280))),
                improj=imp(MG.inp("i2v.improj.x", (2, 1024))),
                resampler_zero_image=res(StandInImageEmbedder(True)(zero)),
                improj_zero_image=imp(StandInImageEmbedder(False)(zero)))


def unet_full_i2v(om):
    import yaml
    with open(os.path.join(MG.REF, "configs/inference_t2v_512_v2.0.yaml")) as f:
        params = dict(yaml.safe_load(f)["model"]["params"]["unet_config"]["params"])
    params.update(use_checkpoint=False, use_image_attention=True)
    MG.unet_cases(om, params, "full_i2v", (4, 16, 40, 64), 1024, [("ctx93", 1, [500], 93, [16])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    om, _ = MG.import_reference()
    T = 8
    MG.unet_cases(om, REDUCED_I2V, "reduced_i2v", (4, T, 16, 16), 128, [
        ("uniform93", 1, [500], 93, 16),                                                  # 77 text + 16 Resampler tokens
        ("frames81", 1, [int(v) for v in np.linspace(999, 0, T).round()], 81, [10]),      # 77 + 4 ImageProjModel tokens, per-frame t
        ("batch2", 2, [981, 20], 93, [10, 24]),
    ])
    projectors()
    if a.full:
        unet_full_i2v(om)


if __name__ == "__main__":
    main()
