"""Trace the sampling layer on the HOST (no GPU): which UNet entry point every guidance call reaches, with which operands, and every
C-ABI launch the samplers issue with its scalars.  `record()` returns {name: array of trace lines | numeric array}; the fixture
tests/golden/sampler_routes.npz holds what the parent commit gives (tools/record_parent_fixtures.py --samplers) and
tests/test_sampler_routes_cpu.py compares this tree with it line by line.

Stand-ins while a trace runs (`tracing()`): `lib.load()` is an object that records every entry point called and returns 0 (it also
WRITES the outputs of moca_cfg_combine_f32 and moca_ddim_update_f32, so a loop's later operands depend on its earlier ones); `lib.ptr`
returns a token of the tensor's dtype, shape and a hash of its content at call time; `ops.current_stream` is a constant;
`torch.empty*` give zeros (a launch that writes nothing must leave something reproducible), `.to("cuda")` stays on the host and
`torch.cuda.current_stream`, `Tensor.record_stream` and `torch.cuda.Event` order nothing.  The step engines of fifo_graph.py run on a
plan that holds buffers only (`BufferPlan`, in place of the module's `_Plan`): no engine method is replaced.  The
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


class HostStream:
    """stands in for a stream and for an event: nothing to order on the host"""
    cuda_stream = 0

    def wait_stream(self, other):
        pass

    def synchronize(self):
        pass

    def record(self, stream=None):
        pass


@contextlib.contextmanager
def tracing(trace):
    from moca_video_amd import lib, ops
    saved = (lib.load, lib.ptr, ops.current_stream, torch.empty, torch.empty_like, torch.Tensor.to, torch.cuda.current_stream,
             torch.Tensor.record_stream, torch.cuda.Event)
    fake = _FakeLib(trace)
    to = torch.Tensor.to
    lib.load = lambda: fake
    lib.ptr = lambda t: None if t is None else _Tok(t)
    ops.current_stream = lambda: 0
    torch.empty, torch.empty_like = torch.zeros, torch.zeros_like
    torch.Tensor.to = lambda self, *a, **k: to(self, *("cpu" if isinstance(x, str) and x == "cuda" else x for x in a), **k)
    torch.cuda.current_stream = lambda device=None: HostStream()
    torch.Tensor.record_stream = lambda self, stream: None
    torch.cuda.Event = HostStream
    try:
        yield
    finally:
        (lib.load, lib.ptr, ops.current_stream, torch.empty, torch.empty_like, torch.Tensor.to, torch.cuda.current_stream,
         torch.Tensor.record_stream, torch.cuda.Event) = saved


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
        adapter_sites = 1

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


# ---- the step engines on a plan that holds buffers only ---------------------------------------------------------------------------
class BufferPlan:
    """what the step engines touch of a `_Plan`, on the host: its buffers, segments, `pieces` and adapter buffers; `set_context` /
    `set_adapter` / `set_concat` record their operands; `_enqueue` / `_ops_stream` order nothing.  The plan's own launch list is ONE
    marker step that writes the line "forward", so a replay shows which of the engine's launches run before the forward and which
    after it."""

    def __init__(self, unet, B, T, H, W, L, in_dtype, device, shared_x=False, pieces=None, adapter=None):
        self.trace, self.B, self.T, self.device = unet.trace, B, T, device
        self.segs = [(B, L)] if isinstance(L, int) else [(int(n), int(l)) for n, l in L]
        self.pieces = None if pieces is None else tuple(int(k) for k in pieces)
        Bx = B // (len(self.segs) if shared_x else 1)
        self.x_in = torch.zeros(Bx, unet.in_channels - sum(self.pieces or ()), T, H, W)
        self.out = torch.zeros(B, 4, T, H, W)
        self.t_rows, self.fps_rows = torch.zeros(B * T, dtype=torch.int64), torch.zeros(B * T, dtype=torch.int64)
        self.adapter_in = None if adapter is None else [torch.zeros(Bx * T, 2, H, W) for _ in range(int(adapter))]
        self.stream = HostStream()
        self.steps = [lambda: self.trace.append("forward")]
        self.trace.append(f"_Plan(B={B},T={T},H={H},W={W},segs={show(self.segs)},shared_x={int(shared_x)},pieces={show(self.pieces)},"
                          f"adapter={show(adapter)})")

    def set_context(self, ctxs):
        self.trace.append(f"set_context({show(ctxs)})")

    def set_adapter(self, features):
        self.trace.append(f"set_adapter({show(features)})")

    def set_concat(self, c_concat):
        self.trace.append(f"set_concat({show(c_concat)})")

    @contextlib.contextmanager
    def _enqueue(self, cur=None):
        yield

    _ops_stream = _enqueue

    def _replay(self):
        for step in self.steps:
            step()

    def close(self):
        self.trace.append("close")


@contextlib.contextmanager
def engine_tracing(trace):
    """`tracing()` with `BufferPlan` under the name the engines construct their plan through -> the module"""
    from moca_video_amd import fifo_graph
    saved, fifo_graph._Plan = fifo_graph._Plan, BufferPlan
    try:
        with tracing(trace):
            yield fifo_graph
    finally:
        fifo_graph._Plan = saved


def _dump(trace, eng, what):
    """what a reset (or `what`) left behind: the device state as the host sees it"""
    trace.append(f"after {what}: state={show(eng.state)} x_in={show(eng.plan.x_in)} fps_rows={show(eng.plan.fps_rows)} coef={show(eng.coef)} "
                 f"t_table={show(eng.t_table)} n_iter={eng.n_iter} it0={getattr(eng, 'it0', '-')}")


EB = 2                                                # latents per engine: "per sample" means something
E_SHAPE = (EB, 4, 2, 2, 2)
E_DDPM_STEPS = 4


def _adapter_maps(seed):
    return [grid((EB * 2, 2, 2, 2), seed)]


def trace_base_engine(which):
    """`BaseEngine`: construction, reset, a step with host-given noise and one without, a second reset with other operands; `which`
    picks the constructor's options and, for "plain", the calls between the two resets"""
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    hybrid = which == "hybrid"
    m = make_model(trace, key="hybrid" if hybrid else "crossattn")
    s = DDIMSampler(m)
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    kw = {"rows": dict(n_rows=T_START), "pred_x0": dict(keep_pred_x0=True), "adapter": dict(features_adapter=_adapter_maps(50))}.get(which, {})
    c, uc = _cond(EB, 3, 16, 1, hybrid), _cond(EB, 3, 16, 2, hybrid)
    with engine_tracing(trace) as fg:
        eng = fg.BaseEngine(m, s, grid(E_SHAPE, 3), c, uc, SCALE, seed=5, **kw)
        _dump(trace, eng, "construction")
        eng.step(noise=grid(E_SHAPE, 6))
        eng.step()
        trace.append(f"latents={show(eng.latents())} last_pred_x0={show(eng.last_pred_x0())}")
        if which == "plain":
            x0 = grid(E_SHAPE, 9)
            for t_index in (3, torch.tensor([2, 4])):
                eng.encode(x0, t_index)
                eng.encode(x0, t_index, noise=grid(E_SHAPE, 11))
                trace.append(f"encoded x_in={show(eng.plan.x_in)} noise={show(eng.noise)}")
            shorter = DDIMSampler(m)
            shorter.make_schedule(T_START, ddim_eta=1.0, verbose=False)
            eng.set_schedule(shorter)
            _dump(trace, eng, "set_schedule")
            eng.step()
            eng.encode(x0, 3)
            init, lpf = grid(E_SHAPE, 12), grid((1, 1, 2, 2, 2), 13)
            eng.reinit(init, lpf, seed=7)
            _dump(trace, eng, "reinit")
            init.add_(1)                              # the same objects again: no upload, so the launches still see the old values
            lpf.add_(1)
            eng.reinit(init, lpf, z_rand=grid(E_SHAPE, 14), seed=8)
            eng.reinit(init.clone(), lpf.clone(), seed=8)
        c2, uc2 = _cond(EB, 3, 8, 7), _cond(EB, 3, 8, 8)
        if hybrid:
            c2["c_concat"] = uc2["c_concat"] = [grid((EB, 2, 2, 2, 2), 41)]
        eng.reset(grid(E_SHAPE, 4), c2, uc2, (1 << 40) + 9, **({"features_adapter": _adapter_maps(51)} if which == "adapter" else {}))
        _dump(trace, eng, "reset")
        if which == "plain":
            eng.reinit(init, lpf, seed=3)             # a reset forgets what was uploaded
        eng.step()
        trace.append(f"n_iter={eng.n_iter} S={eng.S} shape={show(eng.shape)}")
        eng.close()
    return trace


def trace_invert_engine(which):
    from moca_video_amd.sampler import DDIMSampler
    trace = []
    m = make_model(trace)
    s = DDIMSampler(m)
    s.make_schedule(S, ddim_eta=0.0, verbose=False)
    guided = which == "guided"
    c, uc = _cond(EB, 3, 16, 1), _cond(EB, 6, 16, 2) if guided else None
    with engine_tracing(trace) as fg:
        eng = fg.InvertEngine(m, s, grid(E_SHAPE, 3), c, uc, SCALE if guided else 1.0, keep_pred_x0=which == "pred_x0")
        _dump(trace, eng, "construction")
        eng.step()
        eng.step()
        trace.append(f"latents={show(eng.latents())} last_pred_x0={show(eng.last_pred_x0())} t_rows={show(eng.t_rows())} guided={int(eng.guided)}")
        eng.reset(grid(E_SHAPE, 4), _cond(EB, 3, 8, 7), _cond(EB, 6, 8, 8) if guided else None)
        _dump(trace, eng, "reset")
        if which == "unguided":
            for _ in range(S):
                eng.step()
            _run(trace, eng.step)
            trace.append(f"n_iter={eng.n_iter} S={eng.S} zeros={show(eng.zeros)}")
        eng.close()
    return trace


def _mask(which, seed=7):
    return None if which not in ("c0", "full") else (grid((EB, 1 if which == "c0" else 4, 2, 2, 2), seed) > 0).float()


def trace_ddpm_engine(which):
    trace = []
    m = make_model(trace)
    guided = which == "guided"
    c, uc = _cond(EB, 3, 16, 1), _cond(EB, 6, 16, 2) if guided else None
    masked = which in ("c0", "full")
    with engine_tracing(trace) as fg:
        eng = fg.DdpmEngine(m, grid(E_SHAPE, 3), c, uc, SCALE if guided else 1.0, E_DDPM_STEPS, mask=_mask(which), x0=grid(E_SHAPE, 9) if masked else None,
                            seed=5, keep_x_recon=which == "x_recon")
        _dump(trace, eng, "construction")
        eng.step(noise=grid(E_SHAPE, 6), mask_noise=grid(E_SHAPE, 16) if masked else None)
        eng.step()
        trace.append(f"latents={show(eng.latents())} last_x_recon={show(eng.last_x_recon())} t_rows={show(eng.t_rows())} guided={int(eng.guided)} "
                     f"masked={int(eng.masked)} noise={show(eng.noise)}")
        eng.reset(grid(E_SHAPE, 4), _cond(EB, 3, 8, 7), _cond(EB, 6, 8, 8) if guided else None, (1 << 40) + 9, mask=_mask(which, 8),
                  x0=grid(E_SHAPE, 10) if masked else None)
        _dump(trace, eng, "reset")
        eng.step()
        trace.append(f"n_iter={eng.n_iter} S={eng.S} shape={show(eng.shape)}")
        eng.close()
    return trace


def engine_errors():
    """type and message of every refusal of the three engines' constructors, `reset`, `step`, `encode`, `set_schedule` and `reinit`"""
    from moca_video_amd.sampler import DDIMSampler
    trace, lines = [], []
    m = make_model(trace)
    s = DDIMSampler(m)
    s.make_schedule(S, ddim_eta=1.0, verbose=False)
    longer = DDIMSampler(m)
    longer.make_schedule(S + 1, ddim_eta=1.0, verbose=False)
    x, wide = grid(E_SHAPE, 3), grid((EB + 1,) + E_SHAPE[1:], 3)
    c, uc, uc8 = _cond(EB, 3, 16, 1), _cond(EB, 3, 16, 2), _cond(EB, 3, 8, 2)

    def case(name, fn):
        try:
            fn()
            lines.append(f"{name}: no error")
        except Exception as e:
            lines.append(f"{name}: {type(e).__name__}: {e}")
    with engine_tracing(trace) as fg:
        base = fg.BaseEngine(m, s, x, c, uc, SCALE)
        case("base.init.n_rows", lambda: fg.BaseEngine(m, s, x, c, uc, SCALE, n_rows=S + 1))
        case("base.init.fps", lambda: fg.BaseEngine(m, s, x, c, uc8, SCALE))
        case("base.reset.adapter", lambda: base.reset(x, c, uc, features_adapter=_adapter_maps(50)))
        case("base.reset.fps", lambda: base.reset(x, c, uc8))
        case("base.encode.shape", lambda: base.encode(wide, 3))
        case("base.encode.t_shape", lambda: base.encode(x, torch.tensor([1, 2, 3])))
        case("base.encode.t_range", lambda: base.encode(x, S))
        case("base.set_schedule.longer", lambda: base.set_schedule(longer))
        case("base.reinit.initial_noise", lambda: base.reinit(wide, grid((2, 2, 2), 13)))
        case("base.reinit.lpf", lambda: base.reinit(x, grid((2, 2, 3), 13)))
        case("base.reinit.z_rand", lambda: base.reinit(x, grid((2, 2, 2), 13), z_rand=wide))
        inv = fg.InvertEngine(m, s, x, c, uc, SCALE)
        case("invert.init.fps", lambda: fg.InvertEngine(m, s, x, c, uc8, SCALE))
        case("invert.reset.shape", lambda: inv.reset(wide, c, uc))
        case("invert.reset.fps", lambda: inv.reset(x, c, uc8))
        inv.n_iter = S
        case("invert.step.past_S", inv.step)
        ddpm = fg.DdpmEngine(m, x, c, None, 1.0, E_DDPM_STEPS)
        gd = fg.DdpmEngine(m, x, c, uc, SCALE, E_DDPM_STEPS, mask=_mask("c0"), x0=x)
        case("ddpm.init.timesteps", lambda: fg.DdpmEngine(m, x, c, None, 1.0, 0))
        case("ddpm.init.fps", lambda: fg.DdpmEngine(m, x, c, uc8, SCALE, E_DDPM_STEPS))
        case("ddpm.reset.guidance", lambda: ddpm.reset(x, c, uc))
        case("ddpm.reset.mask", lambda: ddpm.reset(x, c, mask=_mask("c0"), x0=x))
        case("ddpm.reset.shape", lambda: ddpm.reset(wide, c))
        case("ddpm.reset.fps", lambda: gd.reset(x, c, uc8, mask=_mask("c0"), x0=x))
        case("ddpm.reset.mask_kind", lambda: gd.reset(x, c, uc, mask=_mask("full"), x0=x))
        case("ddpm.reset.x0", lambda: gd.reset(x, c, uc, mask=_mask("c0"), x0=wide))
        case("ddpm.step.one_draw", lambda: gd.step(noise=x))
    return lines


def _counting(cls, log):
    """a stand-in engine that counts builds, resets and closes; `supported` (and whatever else the class says about a would-be
    constructor call) stays the real class's"""
    class Counting(cls):
        def __init__(self, *a, **k):
            log.append("build")
            sampler = next((v for v in a if hasattr(v, "ddim_timesteps")), None)
            self._shape = next(v for v in a if torch.is_tensor(v)).shape
            self.S, self.it0 = k.get("n_rows") or (len(sampler.ddim_timesteps) if sampler is not None else 0), 0

        def reset(self, *a, **k):
            log.append("reset")
            self.it0 = 0

        def close(self):
            log.append("close")

        def set_schedule(self, sampler):
            self.it0 = self.S - len(sampler.ddim_timesteps)

        def step(self, *a, **k):
            pass

        reinit = step

        def latents(self):
            return torch.zeros(self._shape)
    return Counting


def cache_table():
    """which calls reuse the cached step engine and which build another: `name: <the variant after the base call> <the variant again>`,
    each "hit" (reset only) or "miss" (built; "+close": the cached engine was closed first).  One part of a call varies per line."""
    from moca_video_amd import ddpm as DM
    from moca_video_amd import sampler as SM
    log, lines, trace = [], [], []
    m, mh = make_model(trace), make_model(trace, key="hybrid")
    s, sh = SM.DDIMSampler(m), SM.DDIMSampler(mh)

    on_meta = torch.zeros((1, 4, 2, 2, 2), device="meta")         # (made out here: inside `tracing()` torch.empty is torch.zeros)

    def latent(B=1, meta=False, seed=3):
        return cuda_like(on_meta if meta else grid((B, 4, 2, 2, 2), seed))

    def pair(B, Lc, Lu, pieces=None):
        c, uc = _cond(B, Lc, 16, 1), _cond(B, Lu, 16, 2)
        if pieces is not None:
            c["c_concat"] = uc["c_concat"] = [grid((B, k, 2, 2, 2), 40) for k in pieces]
        return c, uc

    def sample(B=1, Lc=3, Lu=3, scale=SCALE, steps=S, eta=0., meta=False, fa=None, pieces=None, seed=3):
        c, uc = pair(B, Lc, Lu, pieces)
        (s if pieces is None else sh).sample(steps, B, (4, 2, 2, 2), c, eta=eta, x_T=latent(B, meta, seed), unconditional_guidance_scale=scale,
                                             unconditional_conditioning=uc, features_adapter=fa)

    def decode(t_start=T_START):
        s.make_schedule(S, ddim_eta=0., verbose=False)
        c, uc = pair(1, 3, 3)
        s.decode(latent(), c, t_start, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)

    def encode(B=1, Lc=3, Lu=3, scale=1.0, steps=S, eta=0., meta=False, t_enc=3):
        s.make_schedule(steps, ddim_eta=eta, verbose=False)
        c, uc = pair(B, Lc, Lu)
        s.encode(latent(B, meta), c, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=uc)

    def freeinit(steps=(2, 3)):
        c, uc = pair(1, 3, 3)
        s.sample_freeinit(list(steps), 1, (4, 2, 2, 2), grid((1, 1, 2, 2, 2), 13), c, x_T=latent(), unconditional_guidance_scale=SCALE,
                          unconditional_conditioning=uc)

    def loop(B=1, Lc=3, Lu=3, scale=1.0, timesteps=2, mask=None, meta=False, clip=False, param="eps"):
        c, uc = pair(B, Lc, Lu)
        m.clip_denoised, m.parameterization = clip, param
        try:
            mk = None if mask is None else (grid((B, 1 if mask == "c0" else 4, 2, 2, 2), 7) > 0).float()
            m.p_sample_loop(c, (B, 4, 2, 2, 2), x_T=latent(B, meta), timesteps=timesteps, mask=mk, x0=None if mask is None else grid((B, 4, 2, 2, 2), 9),
                            unconditional_guidance_scale=scale, unconditional_conditioning=uc, verbose=False)
        finally:
            m.clip_denoised, m.parameterization = False, "eps"

    def without_scale(fn):
        def call():
            m.use_scale = False
            try:
                fn()
            finally:
                m.use_scale = True
        return call

    def probe(name, base, variant):
        got = []
        for call in (base, variant, variant):
            del log[:]
            call()
            got.append(("miss" if "build" in log else "hit") + ("+close" if "close" in log else ""))
        lines.append(f"{name}: {got[1]} {got[2]}")
    adapter = lambda ch: [grid((2, ch, 2, 2), 50)]
    saved = SM.BaseEngine, SM.InvertEngine, DM.DdpmEngine
    SM.BaseEngine, SM.InvertEngine, DM.DdpmEngine = (_counting(cls, log) for cls in saved)
    try:
        with tracing(trace):
            for name, variant in {"same": sample, "latent_values": lambda: sample(seed=4), "shape": lambda: sample(B=2), "cond_length": lambda: sample(Lc=6),
                                  "uncond_length": lambda: sample(Lu=6), "scale": lambda: sample(scale=2.0), "schedule_length": lambda: sample(steps=S - 1),
                                  "eta": lambda: sample(eta=1.0), "device": lambda: sample(meta=True), "use_scale": without_scale(sample),
                                  "adapter": lambda: sample(fa=adapter(2)), "decode": decode, "decode_all_rows": lambda: decode(S),
                                  "encode": encode, "freeinit": freeinit, "freeinit_same_rows": lambda: freeinit((2, S))}.items():
                probe("sample." + name, sample, variant)
            probe("sample.adapter_shapes", lambda: sample(fa=adapter(2)), lambda: sample(fa=adapter(3)))
            probe("sample.hybrid", sample, lambda: sample(pieces=(2,)))
            probe("sample.concat_widths", lambda: sample(pieces=(2,)), lambda: sample(pieces=(1, 1)))
            probe("decode.n_rows", decode, lambda: decode(T_START - 1))
            for name, variant in {"same": encode, "t_enc": lambda: encode(t_enc=4), "shape": lambda: encode(B=2), "cond_length": lambda: encode(Lc=6),
                                  "guided": lambda: encode(scale=SCALE), "schedule_length": lambda: encode(steps=S - 1), "eta": lambda: encode(eta=1.0),
                                  "device": lambda: encode(meta=True), "use_scale": without_scale(encode), "sample": sample}.items():
                probe("encode." + name, encode, variant)
            guided = lambda **k: encode(scale=SCALE, **k)
            for name, variant in {"uncond_length": lambda: guided(Lu=6), "scale": lambda: encode(scale=2.0)}.items():
                probe("encode.guided." + name, guided, variant)
            for name, variant in {"same": loop, "shape": lambda: loop(B=2), "cond_length": lambda: loop(Lc=6), "guided": lambda: loop(scale=SCALE),
                                  "timesteps": lambda: loop(timesteps=3), "mask_c0": lambda: loop(mask="c0"), "device": lambda: loop(meta=True),
                                  "clip_denoised": lambda: loop(clip=True), "parameterization": lambda: loop(param="x0")}.items():
                probe("p_sample_loop." + name, loop, variant)
            probe("p_sample_loop.mask_kind", lambda: loop(mask="c0"), lambda: loop(mask="full"))
            gloop = lambda **k: loop(scale=SCALE, **k)
            for name, variant in {"uncond_length": lambda: gloop(Lu=6), "scale": lambda: loop(scale=2.0)}.items():
                probe("p_sample_loop.guided." + name, gloop, variant)
            del log[:]
            s.release()
            m.release()
            lines.append("release: " + " ".join(log))
    finally:
        SM.BaseEngine, SM.InvertEngine, DM.DdpmEngine = saved
    return lines


def coefficient_tables():
    """`step_tables` and the `BaseEngine` coefficient table (its constructor run on the host over a plan that holds buffers only)"""
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

        with engine_tracing(trace) as fifo_graph:
            for rows in (None, T_START):
                eng = fifo_graph.BaseEngine(m, s, grid((1, 4, 2, 2, 2), 3), _cond(1, 3, 16, 1), _cond(1, 3, 16, 2), SCALE, n_rows=rows)
                out[f"base_engine.eta{eta:g}.rows{rows}.coef"] = eng.coef.numpy().copy()
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
    for which in ("plain", "rows", "pred_x0", "adapter", "hybrid"):
        out[f"engine.base.{which}"] = trace_base_engine(which)
    for which in ("unguided", "guided", "pred_x0"):
        out[f"engine.invert.{which}"] = trace_invert_engine(which)
    for which in ("unguided", "guided", "c0", "full", "x_recon"):
        out[f"engine.ddpm.{which}"] = trace_ddpm_engine(which)
    out["engine_errors"] = engine_errors()
    out["cache"] = cache_table()
    out.update(coefficient_tables())
    return {k: np.asarray(v) for k, v in out.items()}
