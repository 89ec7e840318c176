#!/usr/bin/env python3
"""Generate the goldens of the two TemporalTransformer variants by running the REAL reference modules on CPU:
`use_causal_attention=True` (attention.py:309-311,342-346,101-105) and `temporal_selfatt_only=False` (:313-314,353-363).

  block_temporal_causal.npz   TemporalTransformer(128 ch, 2 heads, linear, causal, temporal_length = T), weights fill(., 21):
                                a   x [2,128,16,4,5]  (HW = 20: the fused q|k|v + attention launch)
                                b   x [1,128,8,3,5], temporal_length 8  (the standalone kernel, T < 16)
                              (sensitivity condition, asserted here: the same weights WITHOUT the mask give another output.)
  block_temporal_cross.npz    TemporalTransformer(128 ch, 2 heads, linear, only_self_att=False, context_dim 96), weights fill(., 22):
                                a   x [2,128,4,4,4], one 77-token context PER VIDEO (they differ), given as the UNet gives it:
                                    context.repeat_interleave(t)  (openaimodel3d.py:547)
                                b   x [1,128,8,4,4], 154 tokens
  unet_reduced_tvariants.npz  the reduced-width UNet (tools/make_golden.py REDUCED, weights fill(., 11)) with
                                causal        use_causal_attention               x [1,4,16,8,40]   uniform t, 77 tokens
                                causal_fifo   the same model                      x [1,4,16,8,40]   per-frame t, 154 tokens
                                cross         temporal_selfatt_only=False         x [2,4,4,16,16]   two videos, their own 77-token contexts
                                cross154      the same model                      x [1,4,16,32,32]  per-frame t, 154 tokens
                                both          both flags                          x [1,4,8,32,32]   (T != temporal_length: the cross branch
                                                                                                    never uses the mask, :362-363)
                              (sensitivity, asserted here: the non-causal / self-attention-only model with the same weights differs.)
  unet_full_causal.npz        (--full) the YAML's UNet params + use_causal_attention at [1,4,16,40,64], per-frame t, 77 tokens.
  unet_tvariants_keys.npz     (--full) state-dict key / shape lists of the two new full-width configurations, from the reference modules
                              built on the meta device.

    python tools/make_golden_temporal_variants.py [--full | --only-full]

Same recipe as tools/make_golden.py (whose helpers it imports): parameters -- the reference's zero-initialised proj_out included -- and
inputs are regenerated bit-identically from moca_video_amd.weightgen by name, so a fixture holds only expected outputs and call metadata."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
from test_unet_gpu import TOL_BLOCK, TOL_UNET  # noqa: E402

SENS = 20      # the mask must move the output by more than SENS x the test tolerance


def relerr(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def blocks(att):
    out = {}
    with torch.no_grad():
        for name, shape, tl in (("a", (2, 128, 16, 4, 5), 16), ("b", (1, 128, 8, 3, 5), 8)):
            mk = lambda causal: MG.fill(att.TemporalTransformer(128, 2, 64, depth=1, use_linear=True, use_checkpoint=False, only_self_att=True,
                                                                causal_attention=causal, relative_position=False,
                                                                temporal_length=tl).eval(), 21)
            x = MG.inp(f"ttc.{name}.x", shape)
            y, y_plain = mk(True)(x), mk(False)(x)
            sens = relerr(y_plain, y)
            print(f"[block causal] {name}: std {y.std():.4f}; dropping the mask moves it by {sens:.3e} of max|y| (need > {SENS * TOL_BLOCK:.1e})")
            assert sens > SENS * TOL_BLOCK, "the causal mask is not visible in this fixture"
            assert mk(True).proj_out.weight.abs().max() > 0
            out[name] = y
    MG.save("block_temporal_causal", **out)
    out = {}
    with torch.no_grad():
        tt = MG.fill(att.TemporalTransformer(128, 2, 64, depth=1, context_dim=96, use_linear=True, use_checkpoint=False, only_self_att=False,
                                             causal_attention=False, relative_position=False, temporal_length=16).eval(), 22)
        assert tuple(tt.transformer_blocks[0].attn2.to_k.weight.shape) == (128, 96)
        for name, shape, L in (("a", (2, 128, 4, 4, 4), 77), ("b", (1, 128, 8, 4, 4), 154)):
            x = MG.inp(f"ttx.{name}.x", shape)
            ctx = MG.inp(f"ttx.{name}.ctx", (shape[0], L, 96))
            y = tt(x, context=ctx.repeat_interleave(shape[2], dim=0))
            print(f"[block cross] {name}: std {y.std():.4f}")
            out[name] = y
            if name == "a":        # the per-video contexts matter: swapping them moves the output
                y_sw = tt(x, context=ctx.flip(0).repeat_interleave(shape[2], dim=0))
                assert relerr(y_sw, y) > SENS * TOL_BLOCK, "the context is not visible in this fixture"
    MG.save("block_temporal_cross", **out)


def run_unet(model, tag, name, shape, tvals, L, fps, ctx_dim=128):
    x = MG.inp(f"{tag}.{name}.x", shape)
    ctx = MG.inp(f"{tag}.{name}.ctx", (shape[0], L, ctx_dim))
    t = torch.tensor(tvals, dtype=torch.long)
    t0 = time.time()
    y = model(x, t, context=ctx, fps=torch.tensor(fps, dtype=torch.long))
    print(f"[{tag}] {name}: forward {time.time() - t0:.1f}s, out std {y.std():.4f}")
    return {name: y, name + "__t": t, name + "__fps": np.asarray(fps), name + "__L": np.asarray(L)}


def fifo_t(T):
    return [int(v) for v in np.linspace(999, 0, T).round()]


def unets(om):
    out = {}
    mk = lambda **kw: MG.fill(om.UNetModel(**dict(MG.REDUCED, **kw)).eval(), 11)
    with torch.no_grad():
        causal, plain = mk(use_causal_attention=True), mk()
        out.update(run_unet(causal, "tv", "causal", (1, 4, 16, 8, 40), [500], 77, [16]))
        y_plain = run_unet(plain, "tv", "causal", (1, 4, 16, 8, 40), [500], 77, [16])["causal"]
        sens = relerr(y_plain, out["causal"])
        print(f"[tv] causal: dropping the mask moves the output by {sens:.3e} of max|y| (need > {SENS * TOL_UNET:.1e})")
        assert sens > SENS * TOL_UNET, "the causal mask is not visible at the UNet output"
        out.update(run_unet(causal, "tv", "causal_fifo", (1, 4, 16, 8, 40), fifo_t(16), 154, [10]))
        cross = mk(temporal_selfatt_only=False)
        out.update(run_unet(cross, "tv", "cross", (2, 4, 4, 16, 16), [981, 20], 77, [10, 24]))
        out.update(run_unet(cross, "tv", "cross154", (1, 4, 16, 32, 32), fifo_t(16), 154, [10]))
        y_self = run_unet(plain, "tv", "cross", (2, 4, 4, 16, 16), [981, 20], 77, [10, 24])["cross"]
        assert relerr(y_self, out["cross"]) > SENS * TOL_UNET, "the temporal cross-attention is not visible at the UNet output"
        both = mk(temporal_selfatt_only=False, use_causal_attention=True)
        out.update(run_unet(both, "tv", "both", (1, 4, 8, 32, 32), [500], 77, [16]))
    MG.save("unet_reduced_tvariants", **out)


def full_params():
    import yaml
    with open(os.path.join(MG.REF, "configs/inference_t2v_512_v2.0.yaml")) as f:
        params = dict(yaml.safe_load(f)["model"]["params"]["unet_config"]["params"])
    params["use_checkpoint"] = False
    return params


def full_cases(om):
    keys = {}
    for tag, kw in (("causal", dict(use_causal_attention=True)), ("cross", dict(temporal_selfatt_only=False))):
        with torch.device("meta"):
            sd = om.UNetModel(**dict(full_params(), **kw)).state_dict()
        keys[tag + "_keys"] = np.asarray(list(sd))
        keys[tag + "_shapes"] = np.asarray([",".join(str(int(s)) for s in v.shape) for v in sd.values()])
        print(f"[full keys] {tag}: {len(sd)} tensors, {sum(v.numel() for v in sd.values())} parameters")
    MG.save("unet_tvariants_keys", **keys)
    t0 = time.time()
    model = MG.fill(om.UNetModel(**dict(full_params(), use_causal_attention=True)).eval(), 11)
    print(f"[full_causal] reference UNet built+filled in {time.time() - t0:.1f}s")
    with torch.no_grad():
        out = run_unet(model, "full_causal", "fifo16", (1, 4, 16, 40, 64), fifo_t(16), 77, [10], ctx_dim=1024)
    MG.save("unet_full_causal", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--only-full", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(8)
    om, att = MG.import_reference()
    if not a.only_full:
        blocks(att)
        unets(om)
    if a.full or a.only_full:
        full_cases(om)


if __name__ == "__main__":
    main()
