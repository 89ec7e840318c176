"""Trace the sampling layer on the HOST (no GPU): which UNet entry point every guidance call reaches, with which operands, and every
C-ABI launch the samplers issue with its scalars.  `record()` returns {name: array of trace lines | numeric array}; the fixture
tests/golden/sampler_routes.npz holds what the parent commit gives (tools/record_parent_fixtures.py --samplers) and
tests/test_sampler_routes_cpu.py compares this tree with it line by line.

Stand-ins while a trace runs (`tracing()`): `lib.load()` is an object that records every entry point called and returns 0 (it also
WRITES the outputs of moca_cfg_combine_f32 and moca_ddim_update_f32, so a loop's later operands depend on its earlier ones); `lib.ptr`
returns a token of the tensor's dtype, shape and a hash of its content at call time; `ops.current_stream` is a constant;
`torch.empty*` give zeros (a launch that writes nothing must leave something reproducible) and `.to("cuda")` stays on the host.  The
model is the schedule model of tests/v2v_ref.py with the DDPM mixin, a stub wrapper and a stub UNet whose three entry points record
their arguments and return an exact function of ALL of them (x, t, context, fps, adapter maps, c_concat): every operand is a small
dyadic rational, so the sums are exact in fp32 whatever the host's vector width, and a mixed-up operand changes a later hash."""
import contextlib
import ctypes
import hashlib
import types

import numpy as np
import torch

from v2v_ref import ScheduleModel

SCALE = 3.0


def grid(shape, seed):
    """deterministic multiples of 1/8 in [-2, 2]"""
    n = int(np.prod(shape))
    v = ((np.arange(n, dtype=np.int64) * (2 * seed + 7) + 3 * seed) % 33 - 16) / 8.0
    return torch.from_numpy(v.astype(np.float32)).reshape(shape)


class CudaLike(torch.Tensor):
    """a host tensor that answers `is_cuda` with True: what the `supported()` predicates and the DDPM step's routing look at"""
    is_cuda = True


def cuda_like(t):
    return torch.Tensor._make_subclass(CudaLike, t)


def show(v):
    if v is None:
        return "-"
    if torch.is_tensor(v):
        t = v.detach().as_subclass(torch.Tensor).contiguous()
        h = hashlib.sha1(t.numpy().tobytes()).hexdigest()[:10]
        return f"{str(t.dtype)[6:]}[{'x'.join(str(int(s)) for s in t.shape)}]#{h}"
    if isinstance(v, (list, tuple)):
        return "(" + ",".join(show(x) for x in v) + ")"
    if isinstance(v, dict):
        return "{" + ",".join(f"{k}:{show(x)}" for k, x in sorted(v.items())) + "}"
    if isinstance(v, (bool, int, np.integer)):
        return str(int(v))
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    if isinstance(v, np.ndarray):
        return show(torch.from_numpy(np.ascontiguousarray(v)))
    return type(v).__name__


class _Tok:
    def __init__(self, t):
        self.t, self.s = t, show(t)


class _FakeLib:
    def __init__(self, trace):
        self.trace = trace

    def __getattr__(self, name):
        def call(*a):
            self.trace.append(name + "(" + ",".join(
                x.s if isinstance(x, _Tok) else "st" if isinstance(x, ctypes.c_void_p) else show(x) for x in a) + ")")
            if name == "moca_cfg_combine_f32":
                e_c, e_u, out, s = a[0].t, a[1].t, a[2].t, a[3]
                out.copy_(e_u + (e_c - e_u).mul(s))
            if name == "moca_ddim_update_f32":
                x, e, nz, x_prev, pred = (k.t for k in a[:5])
                a_t, a_prev, sig, s1m = (np.float32(k) for k in a[5:9])
                pred.copy_((x - e.mul(float(s1m))).div(float(np.sqrt(a_t))))
                x_prev.copy_(pred.mul(float(np.sqrt(a_prev))) + e.mul(float(np.sqrt(np.float32(1) - a_prev - sig * sig))) + nz.mul(float(sig)))
            return 0
        return call


@contextlib.contextmanager
def tracing(trace):
    from moca_video_amd import lib, ops
    saved = (lib.load, lib.ptr, ops.current_stream, torch.empty, torch.empty_like, torch.Tensor.to)
    fake = _FakeLib(trace)
    to = torch.Tensor.to
    lib.load = lambda: fake
    lib.ptr = lambda t: None if t is None else _Tok(t)
    ops.current_stream = lambda: 0
    torch.empty, torch.empty_like = torch.zeros, torch.zeros_like
    torch.Tensor.to = lambda self, *a, **k: to(self, *("cpu" if isinstance(x, str) and x == "cuda" else x for x in a), **k)
    try:
        yield
    finally:
        lib.load, lib.ptr, ops.current_stream, torch.empty, torch.empty_like, torch.Tensor.to = saved


# ---- the stub model -----------------------------------------------------------------------------------------------------------
def _eps(x, t, ctx, fps, fa=None, concat=None):
    """exact in fp32: x / 4 + t / 1024 + sum_l (l + 1) ctx[:, l] + fps / 64 (+ the adapter maps' and c_concat's sums)"""
    x = x.as_subclass(torch.Tensor)
    B = x.shape[0]
    rows = lambda v: v.reshape(-1, 1, 1, 1, 1)
    tt = torch.as_tensor(t).as_subclass(torch.Tensor).reshape(B, -1).to(torch.float32) / 1024
    out = x.to(torch.float32) / 4 + (rows(tt) if tt.shape[1] == 1 else tt.reshape(B, 1, -1, 1, 1))
    w = torch.arange(1, ctx.shape[1] + 1, dtype=torch.float32).reshape(1, -1, 1)
    out = out + rows((ctx.as_subclass(torch.Tensor).to(torch.float32) * w).sum((1, 2)))
    out = out + (fps / 64 if isinstance(fps, int) else rows(torch.as_tensor(fps).as_subclass(torch.Tensor).reshape(-1).to(torch.float32) / 64))
    for f in fa or ():
        out = out + rows(f.reshape(B, -1).sum(1)) / 16
    for c in concat or ():
        out = out + rows(c.reshape(c.shape[0], -1).sum(1)) / 32
    return out


def _unet_classes():
    from moca_video_amd.unet import UNetModel

    class StubUNet(UNetModel):
        """passes `isinstance(unet, UNetModel)`; nothing of the real model is built"""

        def __init__(self, trace, in_channels=4):
            torch.nn.Module.__init__(self)
            self.trace, self.in_channels, self._packed = trace, in_channels, True

        def _check_adapter(self, fa):
            pass

        def forward_segments(self, x, t, ctxs, fps=None, shared_x=False, features_adapter=None):
            self.trace.append(f"forward_segments(x={show(x)},t={show(t)},ctxs={show(ctxs)},fps={show(fps)},shared_x={int(shared_x)},"
                              f"features_adapter={show(features_adapter)})")
            xs = [x] * len(ctxs) if shared_x else list(x.split([c.shape[0] for c in ctxs], 0))
            return torch.cat([_eps(xi, t, c, f, features_adapter) for xi, c, f in zip(xs, ctxs, fps)], 0)

        def forward_concurrent(self, calls):
            self.trace.append("forward_concurrent(" + ";".join(show(c) for c in calls) + ")")
            return [_eps(c["x"], c["timesteps"], c["context"], c["fps"]) for c in calls]

    class PlainUNet:
        """a foreign UNet: no forward_segments, no forward_concurrent"""
        in_channels = 4

    return StubUNet, PlainUNet


def make_model(trace, key="crossattn", plain_unet=False, use_scale=True):
    from moca_video_amd.ddpm import DdpmMixin
    from moca_video_amd.wrapper import make_beta_schedule
    StubUNet, PlainUNet = _unet_classes()

    class TraceModel(DdpmMixin, ScheduleModel):
        v_posterior, parameterization, clip_denoised, log_every_t = 0., "eps", False, 100

        def _ddpm_t(self, t, x):                      # (the real one refuses host tensors)
            return torch.as_tensor(t).to(torch.int64).contiguous()

        def apply_model(self, x, t, c, **kw):
            trace.append(f"apply_model(x={show(x)},t={show(t)},c={show(c)},kw={show({k: v for k, v in kw.items()})})")
            d = c if isinstance(c, dict) else {"c_crossattn": c if isinstance(c, list) else [c]}
            return _eps(x, t, torch.cat(d["c_crossattn"], 1), d.get("fps", 16), kw.get("features_adapter"), d.get("c_concat"))

        def encode_first_stage_2DAE(self, frames, noise=None):
            trace.append(f"encode_first_stage_2DAE({show(frames)})")
            return frames[:, :3, :, :2, :2].clone()   # 3 channels: the caller pads the fourth

    m = TraceModel()
    m.use_scale = use_scale
    m._betas64 = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
    m.sqrt_alphas_cumprod = torch.sqrt(m.alphas_cumprod)
    m.sqrt_one_minus_alphas_cumprod = torch.sqrt(1 - m.alphas_cumprod)
    m.model = types.SimpleNamespace(conditioning_key=key, diffusion_model=PlainUNet() if plain_unet else StubUNet(trace, 6 if key == "hybrid" else 4))
    return m


# ---- the guidance cases ---------------------------------------------------------------------------------------------------------
def _cond(B, L, fps, seed, concat=False):
    c = {"c_crossattn": [grid((B, L, 8), seed)]}
    if fps is not None:
        c["fps"] = fps
    if concat:
        c["c_concat"] = [grid((B, 2, 2, 2, 2), 40)]
    return c


def guidance_cases():
    """name -> dict(B, c, uc, scale, sampler attributes, model keywords, UNet kwargs, per-frame t)"""
    fa = lambda B: [grid((B * 2, 2, 2, 2), 50)]
    ft = lambda v: torch.tensor([v])
    pair = lambda B=2, Lc=3, Lu=3, fc=16, fu=16, **kw: dict(B=B, c=_cond(B, Lc, fc, 1, kw.pop("concat", False)),
                                                            uc=_cond(B, Lu, fu, 2, kw.pop("uconcat", False)), **kw)
    cases = {
        "no_uc": dict(pair(), uc=None),
        "scale_1": dict(pair(), scale=1.0),
        "equal_int_fps": pair(),
        "equal_tensor_fps": pair(fc=ft(16), fu=ft(16)),
        "no_fps_key": pair(fc=None, fu=None),
        "share_adapter": pair(kw=dict(features_adapter=fa(2))),
        "noshare_int_fps": pair(attrs=dict(share_prefix=False)),
        "noshare_tensor_fps": pair(fc=ft(16), fu=ft(16), attrs=dict(share_prefix=False)),
        "noshare_adapter": pair(attrs=dict(share_prefix=False), kw=dict(features_adapter=fa(2))),
        "concurrent": pair(attrs=dict(cfg_mode="concurrent")),
        "concurrent_no_concurrent": pair(attrs=dict(cfg_mode="concurrent"), kw=dict(no_concurrent=True)),
        "concurrent_adapter": pair(attrs=dict(cfg_mode="concurrent"), kw=dict(features_adapter=fa(2))),
        "len_6_vs_3": pair(Lc=6, Lu=3),
        "len_6_vs_3_noshare": pair(Lc=6, Lu=3, attrs=dict(share_prefix=False)),
        "unequal_int_fps": pair(fc=16, fu=8),
        "unequal_tensor_fps": pair(fc=ft(16), fu=ft(8)),
        "int_vs_tensor_fps": pair(fc=16, fu=ft(16), attrs=dict(share_prefix=False)),
        "hybrid_c_concat": pair(concat=True, uconcat=True, model=dict(key="hybrid")),
        "crossattn_c_concat": pair(concat=True, uconcat=True),
        "B33": pair(B=33),
        "B33_noshare": pair(B=33, attrs=dict(share_prefix=False)),
        "plain_unet": pair(model=dict(plain_unet=True)),
        "plain_unet_concurrent": pair(model=dict(plain_unet=True), attrs=dict(cfg_mode="concurrent")),
        "B1_per_frame_t": pair(B=1, per_frame=True),
        "B1_per_frame_t_noshare": pair(B=1, per_frame=True, attrs=dict(share_prefix=False)),
        "extra_kwargs": pair(kw=dict(clean_cond=True)),
    }
    t3 = pair()
    cases["tensor_cond"] = dict(t3, c=t3["c"]["c_crossattn"][0], uc=t3["uc"]["c_crossattn"][0])
    cases["list_cond"] = dict(t3, c=t3["c"]["c_crossattn"], uc=t3["uc"]["c_crossattn"])
    return cases


def _run(trace, fn):
    try:
        out = fn()
        trace.append("-> " + show(out))
    except Exception as e:                            # a refusal is part of the route
        trace.append(f"raises {type(e).__name__}")


def trace_guidance(case, path):
    """one case through `_cfg_eps`, `unet_windows` (2 windows) or `_ddpm_step`; None where the path does not take the case"""
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    B, c, uc, scale, kw = case["B"], case["c"], case["uc"], case.get("scale", SCALE), case.get("kw", {})
    m = make_model(trace, **case.get("model", {}))
    s = DDIMSampler(m)
    for k, v in case.get("attrs", {}).items():
        setattr(s, k, v)
    x = grid((B, 4, 2, 2, 2), 3)
    t = torch.tensor([999, 500]) if case.get("per_frame") else (torch.arange(B) * 7 + 100)
    if path == "windows" and (B > 2 or not isinstance(c, dict)):
        return None
    if path == "ddpm" and case.get("per_frame"):
        return None
    with tracing(trace):
        if path == "cfg_eps":
            _run(trace, lambda: s._cfg_eps(x, t, c, uc, scale, **kw))
        elif path == "windows":
            one = lambda d: None if d is None else dict(d, c_crossattn=[k[:1] for k in d["c_crossattn"]])
            _run(trace, lambda: s.unet_windows([x[:1], grid((1, 4, 2, 2, 2), 4)], one(c), [np.array([999, 900]), np.array([800, 700])], scale,
                                               one(uc), **kw))
        else:
            _run(trace, lambda: m._ddpm_step(cuda_like(x), c, t, False, want_out=True, noise=grid(x.shape, 5),
                                             unconditional_guidance_scale=scale, unconditional_conditioning=uc, **kw))
    return trace


def supported_table():
    from moca_video_amd.fifo_graph import BaseEngine, DdpmEngine, FifoEngine
    lines = []
    for name, case in guidance_cases().items():
        m = make_model([], **case.get("model", {}))
        c, uc, B = case["c"], case["uc"], case["B"]
        fa = case.get("kw", {}).get("features_adapter")
        for kind, x in (("cuda", cuda_like(grid((B, 4, 2, 2, 2), 3))), ("host", grid((B, 4, 2, 2, 2), 3))):
            row = []
            for fn in (lambda: FifoEngine.supported(m, c, x), lambda: BaseEngine.supported(m, x, c, uc, case.get("scale", SCALE), features_adapter=fa),
                       lambda: DdpmEngine.supported(m, x, c, uc)):
                try:
                    row.append(str(bool(fn())))
                except Exception as e:
                    row.append(type(e).__name__)
            lines.append(f"{name}.{kind}: fifo={row[0]} base={row[1]} ddpm={row[2]}")
    return lines


# ---- loops, steps, queues -------------------------------------------------------------------------------------------------------
S, T_START = 10, 6


def trace_loop(which, eta, use_scale):
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    m = make_model(trace, use_scale=use_scale)
    s = DDIMSampler(m)
    s.use_graph = False
    c, uc = _cond(1, 3, 16, 1), _cond(1, 3, 16, 2)
    x = grid((1, 4, 2, 2, 2), 3)
    noises = [grid(x.shape, 10 + i) for i in range(S)]
    with tracing(trace):
        if which == "sample":
            _run(trace, lambda: s.sample(S, 1, x.shape[1:], c, eta=eta, x_T=x, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc,
                                         noises=noises)[0])
        else:
            s.make_schedule(S, ddim_eta=eta, verbose=False)
            _run(trace, lambda: s.decode(x, c, T_START, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, noises=noises,
                                         use_graph=False))
    return trace


def trace_ddim_step(masks, quirk, cond_channels):
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    s = DDIMSampler(make_model(trace))
    s.reference_index_quirk = quirk
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    shape = (1, 4, 3, 8, 2)                            # H = 8: the clobbered mask index is 1, neither 0 nor the frame's own
    ci = None if cond_channels is None else grid((1, cond_channels, 1, 8, 2), 6)
    with tracing(trace):
        _run(trace, lambda: s.ddim_step(grid(shape, 3), grid(shape, 4), np.array([2, 5, 9]), ci, None, torch.tensor([777, 444, 0]),
                                        davis_masks=(grid((1, 1, 3, 8, 2), 7) > 0).float() if masks else None, noise=grid(shape, 8)))
    return trace


def trace_queue(which, lookahead=False):
    from moca_video_amd.fifo import prepare_latents
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    s = DDIMSampler(make_model(trace))
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    noises = [grid((1, 4, 1, 2, 2), 20 + i) for i in range(S + 2)]
    with tracing(trace):
        if which == "prepare_latents":
            args = types.SimpleNamespace(num_inference_steps=S, video_length=4, lookahead_denoising=lookahead)
            _run(trace, lambda: prepare_latents(args, None, s, initial_latents=grid((1, 4, 4, 2, 2), 9), noises=noises))
        else:
            _run(trace, lambda: s.ddim_inversion(grid((1, 4, 4, 4, 4), 9), S, noises=noises))          # N = 10, T = 4, RGBA frames
    return trace


def trace_fifo(lookahead, batch_windows):
    """two outer iterations of the HOST-driven `fifo_ddim_sampling` (4 steps, windows of 2 frames, masks, guidance): the lookahead
    schedule, the unconditional dict, the window calls and the mask slices.  `shift_latents` (FreeInit: GPU only) is a stand-in that
    records its operands and enqueues the given noise unmixed."""
    from moca_video_amd import fifo
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    m = make_model(trace)
    m.uncond_type = "zero_embed"
    s = DDIMSampler(m)
    s.make_schedule(4, ddim_eta=1.0, verbose=False)
    args = types.SimpleNamespace(num_inference_steps=4, video_length=2, num_partitions=2, lookahead_denoising=lookahead, new_video_length=4)
    Q, nW = (5, 4) if lookahead else (4, 2)

    def shift(latents, davis_data=None, model=None, noise=None, anchor_noise=None):
        trace.append(f"shift_latents({show(latents)},noise={show(noise)})")
        latents[:, :, :-1] = latents[:, :, 1:].clone()
        latents[:, :, -1] = noise.reshape(latents[:, :, -1].shape)
        return latents
    saved, fifo.shift_latents = fifo.shift_latents, shift
    try:
        with tracing(trace):
            _run(trace, lambda: fifo.fifo_ddim_sampling(
                args, m, _cond(1, 3, torch.tensor([8]), 1), (1, 4, 2, 2, 2), s, cfg_scale=SCALE, uc_emb=None if lookahead else grid((1, 3, 8), 2),
                latents=grid((1, 4, Q, 2, 2), 3), conditioned_image=grid((1, 4, 1, 2, 2), 6), masks=(grid((1, 1, Q, 2, 2), 7) > 0).float(),
                n_iterations=2, batch_windows=batch_windows, noises=[[grid((1, 4, 2, 2, 2), 30 + 4 * i + w) for w in range(nW)] for i in range(2)],
                shift_noises=[grid((1, 4, 2, 2), 60 + i) for i in range(2)], use_graph=False))
    finally:
        fifo.shift_latents = saved
    return trace


def coefficient_tables():
    """`step_tables` and the `BaseEngine` coefficient table (its constructor run on the host over a plan that holds buffers only)"""
    from moca_video_amd import fifo_graph
    from moca_video_amd.sampler import DDIMSampler
    out = {}
    for eta in (0.0, 1.0):
        trace = []
        m = make_model(trace)
        s = DDIMSampler(m)
        s.make_schedule(S, ddim_eta=eta, verbose=False)
        for quirk in (True, False):
            s.reference_index_quirk = quirk
            coef, enh, midx = s.step_tables(np.arange(S), np.asarray(s.ddim_timesteps), 8, 3)
            out[f"step_tables.eta{eta:g}.quirk{int(quirk)}.coef"], out[f"step_tables.eta{eta:g}.quirk{int(quirk)}.enh"] = coef, enh
            out[f"step_tables.eta{eta:g}.quirk{int(quirk)}.midx"] = midx

        class BufferPlan:
            def __init__(self, unet, B, T, H, W, *a, **k):
                self.steps, self.x_in, self.out = [], torch.zeros(B // 2, 4, T, H, W), torch.zeros(B, 4, T, H, W)
                self.t_rows = torch.zeros(B * T, dtype=torch.int64)
        saved = fifo_graph._Plan, fifo_graph.BaseEngine.reset
        fifo_graph._Plan, fifo_graph.BaseEngine.reset = BufferPlan, lambda self, *a, **k: None
        try:
            with tracing(trace):
                for rows in (None, T_START):
                    eng = fifo_graph.BaseEngine(m, s, grid((1, 4, 2, 2, 2), 3), _cond(1, 3, 16, 1), _cond(1, 3, 16, 2), SCALE, n_rows=rows)
                    out[f"base_engine.eta{eta:g}.rows{rows}.coef"] = eng.coef.numpy().copy()
        finally:
            fifo_graph._Plan, fifo_graph.BaseEngine.reset = saved
    return out


def record():
    out = {}
    for name, case in guidance_cases().items():
        for path in ("cfg_eps", "windows", "ddpm"):
            tr = trace_guidance(case, path)
            if tr is not None:
                out[f"guidance.{path}.{name}"] = tr
    out["supported"] = supported_table()
    for which in ("sample", "decode"):
        for eta in (0.0, 1.0):
            for use_scale in (True, False):
                out[f"loop.{which}.eta{eta:g}.use_scale{int(use_scale)}"] = trace_loop(which, eta, use_scale)
    for masks in (False, True):
        for quirk in (True, False):
            out[f"ddim_step.masks{int(masks)}.quirk{int(quirk)}"] = trace_ddim_step(masks, quirk, 4)
    out["ddim_step.cond3"] = trace_ddim_step(True, True, 3)
    out["ddim_step.cond_none"] = trace_ddim_step(True, True, None)
    out["ddim_step.cond5"] = trace_ddim_step(True, True, 5)
    out["queue.prepare_latents.lookahead0"] = trace_queue("prepare_latents", False)
    out["queue.prepare_latents.lookahead1"] = trace_queue("prepare_latents", True)
    out["queue.ddim_inversion"] = trace_queue("ddim_inversion")
    for lookahead in (False, True):
        for batch_windows in (False, True):
            out[f"fifo.lookahead{int(lookahead)}.batch_windows{int(batch_windows)}"] = trace_fifo(lookahead, batch_windows)
    out.update(coefficient_tables())
    return {k: np.asarray(v) for k, v in out.items()}
