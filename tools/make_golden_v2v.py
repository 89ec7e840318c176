#!/usr/bin/env python3
"""Generate the video-to-video goldens by running the REAL reference `DDIMSampler` (lvdm/models/samplers/ddim.py) on the CPU:
`stochastic_encode` (:652-671), `decode` (:674-692) and `ddim_inversion` (:972-1032).

  v2v_sample.npz     the real reduced-width UNet inside the real `DiffusionWrapper` through the real `LatentDiffusion.apply_model`, with
                     loop_base's settings (shape [1,4,8,16,16], S = 10, eta 1, guidance 12, use_scale, loop_base's contexts and fps):
                       x_enc = stochastic_encode(x0, [6], noise=n);  x_dec = decode(x_enc, c, 6, 12.0, uc) with six recorded step noises;
                       orig_enc = stochastic_encode(x0b, [999, 0], use_original_steps=True, noise=nb), B = 2.
                     Fixture sensitivity, measured with the reference itself and ASSERTED here: the same x_enc decoded with t_start = 5,
                     and with t_start = 6 but every step's schedule index shifted by one, must each move x_dec by more than
                     3 x TOL_BASE of max|x_dec| (the off-by-one failures of a truncated-table engine stay clear of the tolerance).
  v2v_inversion.npz  the real `ddim_inversion` on a stub model whose `encode_first_stage_2DAE` returns a named z: z [1,4,4,8,8],
                     z [1,3,4,8,8] (the zero-pad branch) and an RGBA input (the stub records the channels it was shown); S = 10,
                     num_inference_steps = 10, the ten torch.randn_like draws are named tensors.
  v2v_cases.npz      index arithmetic recorded from the real methods on a logging FakeModel: the (timestep, index) sequence of
                     `decode` for S = 10, t_start in {1, 6, 10}, and idx(i) of `ddim_inversion` for several (num_inference_steps, T).

    python tools/make_golden_v2v.py

The square roots the two table methods take of fp32 schedule values are pinned to the correctly rounded result (`pinned_sqrt`), so
that the exact goldens do not depend on the CPU the tool ran on.

Same recipe as tools/make_golden.py (whose helpers it imports): parameters and inputs are regenerated bit-identically from
moca_video_amd.weightgen by name, so a fixture holds only the expected outputs and the call metadata."""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(MG.ROOT, "tests"))
from test_loops_gpu import TOL_BASE  # noqa: E402

FACTOR = 3.0                      # sensitivity margin over TOL_BASE
SHAPE = (1, 4, 8, 16, 16)
S, T_START, SCALE = 10, 6, 12.0


def relerr(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def patched_sampler_module():
    from lvdm.models.samplers import ddim as D
    D.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)   # drop the hard-coded .to("cuda") (:53-60)
    D.DDIMSampler.initialize_segmentation_models = lambda self: None
    return D


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


@contextlib.contextmanager
def pinned_sqrt():
    """While the reference's `stochastic_encode` / `ddim_inversion` run, its fp32 `torch.sqrt(t)` and `t ** 0.5` return the correctly
    rounded square root (numpy's: the hardware instruction).  torch's own CPU sqrt is not correctly rounded and its last bit depends
    on the CPU vendor, so without this the coefficients -- and through them every latent of the golden -- would be those of the host
    the tool ran on, and a bit-exact comparison could hold on that host only.  The product takes these coefficients the same way
    (`moca_video_amd.sampler.sqrt_f32`).  `changed` counts the values this host's torch would have rounded the other way."""
    real_sqrt, real_pow = torch.sqrt, torch.Tensor.__pow__
    changed = [0]

    def exact(t, mine):
        out = torch.from_numpy(np.sqrt(t.detach().contiguous().numpy().reshape(-1))).reshape(t.shape)
        changed[0] += int((out != mine).sum())
        return out

    def sqrt(t, *a, **k):
        mine = real_sqrt(t, *a, **k)
        return exact(t, mine) if t.dtype == torch.float32 and not a and not k else mine

    def pow_(self, e):
        mine = real_pow(self, e)
        return exact(self, mine) if self.dtype == torch.float32 and isinstance(e, float) and e == 0.5 else mine
    torch.sqrt, torch.Tensor.__pow__ = sqrt, pow_
    try:
        yield changed
    finally:
        torch.sqrt, torch.Tensor.__pow__ = real_sqrt, real_pow


def sample_case(D, ddpm3d):
    wrapper = ddpm3d.DiffusionWrapper({"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(MG.REDUCED)},
                                      "crossattn").eval()
    MG.fill(wrapper.diffusion_model, 11)

    class Model(MG.FakeModel):
        model = wrapper
        apply_model = ddpm3d.LatentDiffusion.apply_model

    model = Model()
    fps = torch.tensor([10])
    cond = {"c_crossattn": [MG.inp("loop.ctx1", (1, 77, 128))], "fps": fps}
    uc = {"c_crossattn": [MG.inp("loop.uctx", (1, 77, 128))], "fps": fps}
    x0 = MG.inp("v2v.x0", SHAPE)
    n_enc = MG.inp("v2v.enc_noise", SHAPE)
    noises = [MG.inp(f"v2v.noise{i}", SHAPE) for i in range(T_START)]
    s = D.DDIMSampler(model)
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    real = D.noise_like

    def decode(t_start, shift=0, shift_t=False):
        q = list(noises)
        D.noise_like = lambda shp, dev, repeat=False: q.pop(0).clone()
        orig = s.p_sample_ddim

        def shifted(x, c, t, index, **kw):
            if shift_t:
                t = torch.full_like(t, int(s.ddim_timesteps[index + shift]))
            return orig(x, c, t, index=index + shift, **kw)
        if shift:
            s.p_sample_ddim = shifted
        try:
            with torch.no_grad(), quiet():
                out = s.decode(x_enc, cond, t_start, SCALE, uc)
        finally:
            D.noise_like = real
            if shift:
                del s.p_sample_ddim
        assert len(q) == T_START - t_start, "decode drew another number of noises than steps"
        return out

    with torch.no_grad(), pinned_sqrt() as changed:
        x_enc = s.stochastic_encode(x0, torch.tensor([T_START]), noise=n_enc)
    print(f"[v2v] stochastic_encode: {changed[0]} of the table's square roots differ from this host's torch")
    t0 = time.time()
    x_dec = decode(T_START)
    print(f"[v2v] decode {T_START} steps: {time.time() - t0:.1f}s, x_enc std {x_enc.std():.3f}, x_dec std {x_dec.std():.3f} "
          f"max {x_dec.abs().max():.2f}")
    # ---- fixture sensitivity (the reference against itself)
    need = FACTOR * TOL_BASE
    moved = {"t_start - 1": relerr(decode(T_START - 1), x_dec),
             "index + 1": relerr(decode(T_START, shift=1), x_dec),
             "index + 1 and its timestep": relerr(decode(T_START, shift=1, shift_t=True), x_dec)}
    for k, v in moved.items():
        print(f"[v2v] sensitivity, {k}: x_dec moves by {v:.3e} of max|x_dec| (need > {need:.2e}, margin {v / need:.1f} x)")
    assert all(v > need for v in moved.values()), "the fixture does not separate an off-by-one decode from TOL_BASE: change the fixture"
    # ---- use_original_steps: the sampler's own 1000-entry tables
    shape_b = (2, 4, 4, 8, 8)
    with torch.no_grad():
        orig_enc = s.stochastic_encode(MG.inp("v2v.orig.x0", shape_b), torch.tensor([999, 0]), use_original_steps=True,
                                       noise=MG.inp("v2v.orig.noise", shape_b))
    MG.save("v2v_sample", x_enc=x_enc, x_dec=x_dec, orig_enc=orig_enc, t_start=np.asarray(T_START), S=np.asarray(S),
            scale=np.asarray(SCALE), sens=np.asarray(list(moved.values())))


def inversion_case(D):
    class Stub(MG.FakeModel):
        z = None
        seen = None

        def encode_first_stage_2DAE(self, frames):
            self.seen = tuple(frames.shape)
            return self.z.clone()

    model = Stub()
    s = D.DDIMSampler(model)
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    real = torch.randn_like
    out = {}
    for case, zc, fc in (("z4", 4, 3), ("z3", 3, 3), ("rgba", 4, 4)):
        model.z = MG.inp(f"v2v.inv.{case}.z", (1, zc, 4, 8, 8))
        frames = MG.inp(f"v2v.inv.{case}.frames", (1, fc, 4, 64, 64))
        k = [0]

        def named(t, *a, **kw):
            n = MG.inp(f"v2v.inv.{case}.nz{k[0]}", tuple(t.shape))
            k[0] += 1
            return n
        torch.randn_like = named
        try:
            with torch.no_grad(), pinned_sqrt() as changed:
                lat = s.ddim_inversion(frames, 10)
        finally:
            torch.randn_like = real
        print(f"[v2v] ddim_inversion {case}: {changed[0]} of the 20 coefficients differ from this host's torch")
        assert k[0] == 10 and lat.shape == (1, 4, 10, 8, 8)
        out[case] = lat
        out[case + "__seen"] = np.asarray(model.seen)
        print(f"[v2v] ddim_inversion {case}: encoder saw {model.seen}, out {tuple(lat.shape)} std {lat.std():.3f}")
    MG.save("v2v_inversion", **out)


def index_cases(D):
    """(timestep, index) of every `decode` step and idx(i) of `ddim_inversion`, logged from the real methods"""
    log = []

    class Logger(MG.FakeModel):
        def apply_model(self, x, t, c, **kw):
            log.append(int(t[0]))
            return torch.zeros_like(x)

        def encode_first_stage_2DAE(self, frames):       # latent frame k holds k + 1
            T = frames.shape[2]
            return (torch.arange(T, dtype=torch.float32) + 1).reshape(1, 1, T, 1, 1).expand(1, 4, T, 2, 2).clone()

    model = Logger()
    s = D.DDIMSampler(model)
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    out = {}
    orig = s.p_sample_ddim
    idx_log = []

    def spy(x, c, t, index, **kw):
        idx_log.append(int(index))
        return orig(x, c, t, index=index, **kw)
    s.p_sample_ddim = spy
    for t_start in (1, 6, 10):
        log.clear(); idx_log.clear()
        with torch.no_grad(), quiet():
            s.decode(torch.zeros(1, 4, 2, 2, 2), None, t_start)
        assert len(log) == len(idx_log) == t_start
        out[f"decode_S{S}_t{t_start}"] = np.asarray([log, idx_log], dtype=np.int64)          # [2][t_start]: timesteps, indices
        print(f"[v2v] decode t_start={t_start}: timesteps {log} indices {idx_log}")
    del s.p_sample_ddim
    real = torch.randn_like
    torch.randn_like = lambda t, *a, **kw: torch.zeros(t.shape)
    try:
        for N, T in ((10, 4), (10, 10), (10, 12), (6, 4), (3, 1)):
            with torch.no_grad():
                lat = s.ddim_inversion(torch.zeros(1, 3, T, 8, 8), N)
            a = torch.as_tensor(np.asarray(s.ddim_alphas), dtype=torch.float32)[:N] ** 0.5
            idx = (lat[0, 0, :, 0, 0] / a).round().long() - 1
            out[f"inversion_N{N}_T{T}"] = idx.numpy().astype(np.int64)
            print(f"[v2v] ddim_inversion N={N} T={T}: idx {idx.tolist()}")
    finally:
        torch.randn_like = real
    MG.save("v2v_cases", **out)


def main():
    torch.set_num_threads(8)
    MG.import_reference()
    from lvdm.models import ddpm3d
    D = patched_sampler_module()
    index_cases(D)
    inversion_case(D)
    sample_case(D, ddpm3d)


if __name__ == "__main__":
    main()
