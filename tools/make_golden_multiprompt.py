#!/usr/bin/env python3
"""Generate tests/golden/loop_fifo_multiprompt.npz by running the REAL `fifo_ddim_sampling_multiprompts`
(scripts/evaluation/funcs.py:375-468) on CPU, with the recipe of tools/make_golden.py::loop_cases (whose helpers it imports):
the real reduced-width UNet inside the real `DiffusionWrapper`, the real reduced-width `AutoencoderKL`, the real
`LatentDiffusion.apply_model` / `decode_first_stage_2DAE` on a holder, every torch.randn / randn_like / noise_like draw replaced
by a named weightgen tensor, `.to("cuda")` a no-op and the text encoder a table of named embeddings.

The case: prompt mode, S = 16, f = 8, 2 partitions, lookahead (queue of 20 frames, 4 windows), CFG 3, two prompts with
frame counts "2,3" and `trange` cut to 12 iterations: the first S - f = 8 iterations and 2 more use prompt 0, the switch
happens at iteration 10, iterations 10 and 11 use prompt 1.  CFG 3, not loop_fifo's 12: guidance multiplies the fp16 UNet's
error by the scale in every one of the 12 fed-back iterations, and at 12 the drift of the first 8 alone exceeds the tests' 3e-2
bound (4.2e-2 at iteration 8).  `cond_image=` and `target=` go through **kwargs to `fifo_onestep`, so every window takes
`ddim_step`'s segmentation branch with the scripted Grounded-SAM-2 masks of tests/helpers.py::loop_sam_candidates (call index = 4 * iteration + window).

Recorded: the segment index of every iteration, x_prev / pred_x0 of the `ddim_step` calls of iterations 8 .. 11 (the two on
either side of the switch; float16, which keeps the fixture under 1 MiB and sits far below the test tolerance), the latent frame
each iteration emits (the input of `decode_first_stage_2DAE`), the queue after the last shift and the number of draws.

    python tools/make_golden_multiprompt.py
"""
import contextlib
import io
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

TAG = "loop.fifo_mp.prompt"
N_ITER = 12                       # the trange cut
REC_FROM = 8                      # per-call outputs are kept from this iteration on
MULTIPROMPTS = ["a prompt", "a conditioned prompt", "2,3"]
CFG = 3.0


def main():
    torch.set_num_threads(8)
    MG.import_reference()
    stub_t = sys.modules["torchvision"]
    sys.modules["torchvision.transforms"] = stub_t.transforms
    from scripts.evaluation import funcs as Fn
    from lvdm.models.samplers import ddim as D
    from lvdm.models import ddpm3d
    from lvdm.models.autoencoder import AutoencoderKL
    D.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    D.DDIMSampler.initialize_segmentation_models = lambda self: None

    unet_cfg = {"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(MG.REDUCED)}
    wrapper = ddpm3d.DiffusionWrapper(unet_cfg, "crossattn").eval()
    MG.fill(wrapper.diffusion_model, 11)
    ae = AutoencoderKL(ddconfig=dict(MG.VAE_DD, ch=64), lossconfig={"target": "torch.nn.Identity"}, embed_dim=4).eval()
    MG.fill(ae, seed=5)
    text = {"a prompt": MG.inp("loop.ctx1", (1, 77, 128)), "a conditioned prompt": MG.inp("loop.ctx2", (1, 77, 128)),
            "": MG.inp("loop.uctx", (1, 77, 128))}
    embeds = []                                       # what get_learned_conditioning handed out, in call order

    class LoopModel(MG.FakeModel):
        uncond_type = "empty_seq"
        scale_factor = 0.18215
        first_stage_model = ae
        model = wrapper
        apply_model = ddpm3d.LatentDiffusion.apply_model
        decode_first_stage_2DAE = ddpm3d.LatentDiffusion.decode_first_stage_2DAE

        def get_learned_conditioning(self, prompts):
            # funcs.py:382 hands over ONE string per prompt, :399 a list for the empty prompt
            e = torch.cat([text[p] for p in ([prompts] if isinstance(prompts, str) else prompts)], 0).clone()
            embeds.append(e)
            return e

    model = LoopModel()
    real = dict(randn=torch.randn, randn_like=torch.randn_like, to=torch.Tensor.to, noise_like=D.noise_like, trange=Fn.trange)
    counters = {}

    def named(kind, shape):
        k = counters.get(kind, 0)
        counters[kind] = k + 1
        return MG.inp(f"{TAG}.{kind}{k}", tuple(shape))

    def to_nocuda(self, *a, **k):
        if a and isinstance(a[0], str) and a[0] == "cuda":
            return real["to"](self, **k) if k else self
        return real["to"](self, *a, **k)

    def rec_randn(*shape, **k):
        shp = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        return named("randn", shp)

    def patch():
        torch.randn = rec_randn
        torch.randn_like = lambda t, *a, **k: named("randn_like", t.shape)
        torch.Tensor.to = to_nocuda
        D.noise_like = lambda shp, dev, repeat=False: named("noise_like", shp)
        Fn.trange = lambda n, **k: range(min(n, N_ITER))

    def unpatch():
        torch.randn, torch.randn_like, torch.Tensor.to = real["randn"], real["randn_like"], real["to"]
        D.noise_like, Fn.trange = real["noise_like"], real["trange"]

    class Cond(dict):
        """the caller's conditioning dict: funcs.py:430 rewrites its context once per iteration -- note which segment"""
        segments = []

        def update(self, other):
            e = other["c_crossattn"][0]
            self.segments.append(next(k for k, x in enumerate(embeds) if x is e))
            return super().update(other)

    args = types.SimpleNamespace(num_inference_steps=16, video_length=8, lookahead_denoising=True, num_partitions=2,
                                 new_video_length=10, save_frames=False)
    shape = [1, 4, 8, 16, 16]
    cimg = (MG.inp("loop.cimg", (1, 4, 1, 16, 16)) * 0.25 + 0.5).clamp(0, 1)
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp()
    os.chdir(tmp)
    try:
        torch.save(MG.inp("loop.z16", (1, 4, 8, 16, 16)), os.path.join(tmp, "16.pt"))
        s = D.DDIMSampler(model)
        s.make_schedule(ddim_num_steps=16, ddim_eta=1.0, verbose=False)

        class Proc:
            cands, k = None, 0

            def __call__(self, images=None, text=None, return_tensors="pt"):
                return {"input_ids": torch.zeros(1, 4, dtype=torch.int64), "pixel_values": torch.zeros(1, 3, 2, 2)}

            def post_process_grounded_object_detection(self, outputs, input_ids, box_threshold=0.4, text_threshold=0.3, target_sizes=None):
                c = self.cands[self.k]
                return [{"boxes": torch.zeros(0 if c is None else c.shape[0], 4)}]

        class Pred:
            def set_image(self, img):
                assert img.ndim == 3 and img.shape[2] == 3 and img.dtype == np.uint8

            def predict(self, point_coords=None, point_labels=None, box=None, multimask_output=False):
                c = proc.cands[proc.k]
                assert box.shape[0] == c.shape[0]
                return c.numpy().copy(), None, None
        proc = Proc()
        s.processor, s.sam2_predictor, s.grounding_model = proc, Pred(), (lambda **kw: None)
        orig_seg, orig_step = s._apply_segmentation, s.ddim_step
        seen, steps = [], []

        def counted(pred_x0, cond_image, target, step, pre_masks):
            proc.k = seen[-1]["frames"][len(seen[-1]["out"])]
            res = orig_seg(pred_x0, cond_image, target, step, pre_masks)
            seen[-1]["out"].append(int(res[0].shape[2]))
            return res
        s._apply_segmentation = counted

        def spy_step(sample, noise_pred, indices, cond_image, target, ts, **kw):
            assert target == "object." and cond_image is cimg and kw.get("davis_masks") is None
            call = len(steps)
            F = sample.shape[2]
            proc.cands = MG.loop_sam_candidates(call, F, sample.shape[3], sample.shape[4])
            seen.append({"frames": [i for i in range(F) if int(ts[i]) <= 300], "out": []})
            xp, p0 = orig_step(sample, noise_pred, indices, cond_image, target, ts, **kw)
            counts = [1] * F                 # fold the frame replication of injected frames (see make_golden.py::loop_cases)
            for fr, n in zip(seen[-1]["frames"], seen[-1]["out"]):
                counts[fr] = n
            parts, o = [], 0
            for n in counts:
                blk = p0[:, :, o:o + n]
                for j in range(1, n):
                    assert torch.equal(blk[:, :, [j]], blk[:, :, [0]])
                parts.append(blk[:, :, [0]])
                o += n
            assert o == p0.shape[2]
            steps.append((xp.clone(), torch.cat(parts, 2)))
            return xp, p0
        s.ddim_step = spy_step

        emitted, shifts = [], []
        orig_dec, orig_shift = LoopModel.decode_first_stage_2DAE, Fn.shift_latents

        def spy_dec(self, z, **kw):
            emitted.append(z.clone())
            return orig_dec(self, z, **kw)

        def spy_shift(latents, *a, **k):
            r = orig_shift(latents, *a, **k)
            shifts.append(r.clone())
            return r
        LoopModel.decode_first_stage_2DAE, Fn.shift_latents = spy_dec, spy_shift
        patch()
        t0 = time.time()
        try:
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                cond = Cond({"c_crossattn": [model.get_learned_conditioning(["a prompt"])], "fps": torch.tensor([10])})
                embeds.clear()
                Fn.fifo_ddim_sampling_multiprompts(args, model, cond, shape, s, list(MULTIPROMPTS), cfg_scale=CFG, output_dir=tmp,
                                                   latents_dir=tmp, save_frames=False, cond_image=cimg, target="object.")
        finally:
            LoopModel.decode_first_stage_2DAE, Fn.shift_latents = orig_dec, orig_shift
            unpatch()
        draws = dict((k, v) for k, v in counters.items())
        seg = np.asarray(Cond.segments)
        print(f"loop fifo multiprompt: {time.time() - t0:.1f}s, {len(steps)} ddim_step calls, {len(shifts)} shifts, draws {draws}, "
              f"segments {seg.tolist()}")
        assert len(steps) == 4 * N_ITER and len(shifts) == N_ITER and len(emitted) == N_ITER
        assert seg.tolist() == [0] * 10 + [1] * 2
        out = {f"n_{k}": np.asarray(v) for k, v in draws.items()}
        MG.save("loop_fifo_multiprompt", segment=seg, multiprompts=np.asarray(MULTIPROMPTS), n_iterations=np.asarray(N_ITER), cfg_scale=np.asarray(CFG),
                rec_from=np.asarray(REC_FROM),
                x_prev=torch.stack([a for a, _ in steps[4 * REC_FROM:]]).half(),
                pred_x0=torch.stack([b for _, b in steps[4 * REC_FROM:]]).half(),
                frames=torch.cat(emitted, 2), queue=shifts[-1], **out)
    finally:
        unpatch()
        os.chdir(cwd)


if __name__ == "__main__":
    main()
