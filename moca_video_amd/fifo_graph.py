"""One outer iteration of `fifo_ddim_sampling` (scripts/evaluation/funcs.py:305-371) as ONE hipGraph.

The reference walks the 2n windows of an iteration one after the other (clone the window, two UNet forwards, ddim_step with
~100 tiny torch ops per frame, write the second half back), decodes, then shifts the queue by cloning it.  Here everything an
iteration needs lives on the device and depends on nothing the host has to look at:

  * the latent queue is a ring [C][Q][HW] f32 whose head / iteration counter / RNG seed sit in a 32-byte state block
    (`moca_fifo_state`); a shift is `head += 1`, the FreeInit-mixed frame overwrites the dequeued frame's slot;
  * timesteps, DDIM coefficients, mask-frame indices and enhancement factors depend on the window slot only (funcs.py:290-312):
    built once as device tables;
  * the noise of ddim.py:561 / funcs.py:92 comes from a Philox kernel keyed by (seed, iteration) -- or from the caller, for
    fixtures;
  * the 2n conditional windows (two prompts: 154 tokens) and their 2n unconditional copies (77 tokens) are ONE UNet forward of
    batch 4n with two context segments (`_Plan.segs`);
  * classifier-free guidance, the MoCA ddim_step of all windows, the write-back, the emission, the FreeInit mix and the queue /
    mask shift are five more launches on the same stream.

The recorded sequence (gather + ~640 UNet launches + tail) is run eagerly once, captured on the second iteration and replayed
as one `hipGraphLaunch` from then on; the host never synchronises inside the loop.

The module's classes: `_StepEngine` (the wrap of a plan's recorded forward into an engine's launches, one enqueue per step, the
accessors) under all four engines; `FifoEngine`, the loop above; `_TrajectoryEngine` under the three engines that step B latents in the
plan's input buffer by one schedule-table row per replay -- `BaseEngine` (DDIM sampling), `InvertEngine` (DDIM inversion), `DdpmEngine`
(`p_sample_loop`) -- which owns the one- or two-branch plan, the reset core, the launches around the forward and the shared clauses
of `supported()`.  Each of the three says beside `supported()` what a built engine is good for (`key`), which is what `EngineCache`
compares.  `DpmEngine` is `BaseEngine` with the tables and the step of DPM-Solver++(2M) (`dpmpp_tables`): same launches around the
forward, the multistep bit in the step's flag word, no draw.  Both take `mask=` / `x0=` (inpainting): a masked engine launches
`moca_ddpm_step_f32` in its blend-only mode on the latents in front of the forward, behind a draw that covers q_sample's noise too."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np
import torch

from . import lib as _l
from . import ops
from .conditioning import (check_schedule_index, cond_image_rows, conditioning_key, as_cond_dict, context, fps_rows, one_fps,
                           refuse_concat, refuse_image_attention, refuse_long_window, same_fps, unet_of)
from .freeinit import get_freq_filter
from .plan import _Plan
from .unet import UNetModel


def fifo_windows(args):
    """Window schedule of one outer iteration (funcs.py:290-312): (start, mid, end) for rank = 2n-1 .. 0 (reversed so every
    window reads only not-yet-rewritten frames)."""
    f = args.video_length
    n = 2 * args.num_partitions if args.lookahead_denoising else args.num_partitions
    for rank in reversed(range(n)):
        start = rank * (f // 2) if args.lookahead_denoising else rank * f
        yield start, start + f // 2, start + f


def lookahead_schedule(sampler, args):
    """(timesteps, indices) per queue frame (funcs.py:290-294): the schedule's, behind video_length // 2 copies of its first entry
    when the loop denoises with lookahead"""
    timesteps, indices = np.asarray(sampler.ddim_timesteps), np.arange(args.num_inference_steps)
    if args.lookahead_denoising:
        n_look = args.video_length // 2
        timesteps = np.concatenate([np.full((n_look,), timesteps[0]), timesteps])
        indices = np.concatenate([np.full((n_look,), 0), indices])
    return timesteps, indices


def ddim_coef(sampler, index):
    """the five coefficients of schedule index `index` that every DDIM step kernel reads -- sqrt(a_t), sqrt(a_prev), sigma_t,
    sqrt(1 - a_t), sqrt(1 - a_prev - sigma_t^2) -- evaluated in fp32 exactly as the reference's 0-dim tensors are
    (ddim.py:331-343,409-418)"""
    f32 = np.float32
    a_t, a_prev, sig = f32(sampler.ddim_alphas[index]), f32(sampler.ddim_alphas_prev[index]), f32(sampler.ddim_sigmas[index])
    return np.sqrt(a_t), np.sqrt(a_prev), sig, f32(sampler.ddim_sqrt_one_minus_alphas[index]), np.sqrt(f32(1.) - a_prev - sig * sig)


def invert_coef(sampler, i):
    """the coefficients of DDIM inversion step `i`, which takes the latents from schedule level ddim_alphas_prev[i] (a_cur) up to
    ddim_alphas[i] (a_next) with the model evaluated at ddim_timesteps[i]: the tail of p_sample_ddim (ddim.py:328-357) with its tables
    swapped and sigma 0.  -> the five of `ddim_coef` in its order -- sqrt(a_cur), sqrt(a_next), 0, sqrt(1 - a_cur), sqrt(1 - a_next) --
    and the two scales (s_cur, s_next) = (ddim_scale_arr_prev[i], ddim_scale_arr[i]), 1 without `use_scale`: a row of the 8-wide step
    table.  fp32 scalars with correctly rounded roots like `ddim_coef`'s; sqrt(1 - a_cur) is built the way the reference builds
    `ddim_sqrt_one_minus_alphas` (ddim.py:88), as np.sqrt(1. - ddim_alphas_prev), and then taken as fp32."""
    f32 = np.float32
    a_cur, a_next = f32(sampler.ddim_alphas_prev[i]), f32(sampler.ddim_alphas[i])
    s1m_cur = f32(np.sqrt(1. - np.asarray(sampler.ddim_alphas_prev))[i])
    if bool(sampler.use_scale):
        s_cur, s_next = f32(sampler.ddim_scale_arr_prev[i]), f32(sampler.ddim_scale_arr[i])
    else:
        s_cur = s_next = f32(1)
    return np.sqrt(a_cur), np.sqrt(a_next), f32(0), s1m_cur, np.sqrt(f32(1.) - a_next), s_cur, s_next


def dpmpp_tables(sampler, n_rows, order=2, lower_order_final=True):
    """The step tables of DPM-Solver++(2M) (Lu et al., 2022; data prediction, midpoint form) over the first `n_rows` rows of the
    sampler's eta-0 schedule -> (coef [n_rows][8] fp32 = {sqrt(a_t), c_0, c_1, sqrt(1 - a_t), c_x, scale_t, 0, 0}, the int64 timesteps):
    the second row layout of `moca_base_ddim_step_f32` (MOCA_BASE_MULTISTEP).  Row i takes the latents from level (a, s) =
    (ddim_alphas[i], ddim_scale_arr[i]) to (ddim_alphas_prev[i], ddim_scale_arr_prev[i]), s = 1 without `use_scale`; with
    alpha = sqrt(a) s, sigma = sqrt(1 - a), lam = log(alpha / sigma) and h = lam_prev - lam, in float64 rounded to fp32 once:

        c_x = sigma_prev / sigma      c_0 = -alpha_prev expm1(-h)      c_1 = 0.5 c_0 h / h_prev      x' = c_x x + c_0 p0 + c_1 (p0 - p0_prev)

    Columns 0, 3 and 5 are `ddim_coef`'s and `BaseEngine`'s, so pred_x0 has DDIM's bits.  A trajectory walks the rows from n_rows - 1
    down.  A row with h == 0 is an identity row (c_x = 1, c_0 = c_1 = 0): every `uniform` schedule has one at i = 0, and the identity
    rows at the clean end are not stepped at all (`dpm_stepped_rows`).  c_1 is 0 -- first order, the history is not read -- on the
    first stepped row, on every row with `order` 1 and, with `lower_order_final`, on the last stepped row; h_prev is the h of the row
    above.  An identity row ABOVE a stepped one (repeated timesteps, as 'quad' discretisation makes them) would put its own p0 into
    the history at a distance h_prev = 0: refused."""
    if order not in (1, 2):
        raise ValueError(f"order = {order}: DPM-Solver++ multistep is built for orders 1 and 2")
    n_rows = int(n_rows)
    if not 1 <= n_rows <= len(sampler.ddim_timesteps):
        raise ValueError(f"n_rows = {n_rows}: the schedule has {len(sampler.ddim_timesteps)} rows")
    if np.any(np.asarray(sampler.ddim_sigmas, dtype=np.float64) != 0):
        raise ValueError("dpmpp_tables: the solver is deterministic, its schedule is made with eta 0")
    f64 = lambda v: np.asarray(v, dtype=np.float64)[:n_rows]
    a, ap = f64(sampler.ddim_alphas), f64(sampler.ddim_alphas_prev)
    use_scale = bool(sampler.use_scale)
    sc, scp = (f64(sampler.ddim_scale_arr), f64(sampler.ddim_scale_arr_prev)) if use_scale else (np.ones(n_rows), np.ones(n_rows))
    alpha_p, sigma, sigma_p = np.sqrt(ap) * scp, np.sqrt(1. - a), np.sqrt(1. - ap)
    h = np.log(alpha_p / sigma_p) - np.log(np.sqrt(a) * sc / sigma)
    stepped = np.flatnonzero(h != 0)
    first = int(stepped[0]) if stepped.size else n_rows          # the identity rows at the clean end: 0 .. first - 1
    if np.any(h[first:] == 0):
        raise ValueError("dpmpp_tables: schedule rows with equal levels (repeated timesteps) above the clean end")
    coef = np.zeros((n_rows, 8), np.float32)
    for i in range(n_rows):
        coef[i, 0], _, _, coef[i, 3], _ = ddim_coef(sampler, i)
        coef[i, 5] = sampler.ddim_scale_arr[i] if use_scale else 1.0
        coef[i, 4] = 1.0
        if i < first:
            continue
        c_0 = -alpha_p[i] * np.expm1(-h[i])
        coef[i, 1], coef[i, 4] = c_0, sigma_p[i] / sigma[i]
        if order == 2 and i < n_rows - 1 and not (lower_order_final and i == first):
            coef[i, 2] = 0.5 * c_0 * h[i] / h[i + 1]
    t_table = np.ascontiguousarray(np.asarray(sampler.ddim_timesteps, dtype=np.int64)[:n_rows])
    return torch.from_numpy(coef), torch.from_numpy(t_table)


def dpm_stepped_rows(coef):
    """how many rows of a `dpmpp_tables` table a trajectory steps: all but the identity rows at the clean end (one forward saved each)"""
    c = np.asarray(coef)
    identity = (c[:, 1] == 0) & (c[:, 2] == 0) & (c[:, 4] == 1)
    return int(c.shape[0] - (np.argmin(identity) if not identity.all() else c.shape[0]))


def n_ctx(cond):
    """the tokens of a cond dict's cross-attention context (`context(cond)`: its `c_crossattn` entries side by side)"""
    return sum(int(k.shape[1]) for k in cond["c_crossattn"])


class EngineCache:
    """one cached step engine and what it was built for: `entry` is None or (key, engine)"""
    entry = None

    def get(self, key, build, reset):
        """the engine for `key` at the start of a new trajectory: the cached one after `reset(engine)`, or -- the cached one closed if
        its key is another -- `build()`"""
        if self.entry is not None and self.entry[0] != key:
            self.release()
        if self.entry is None:
            self.entry = (key, build())
        else:
            reset(self.entry[1])
        return self.entry[1]

    def release(self):
        """close the cached engine (plan buffers + hipGraph)"""
        if self.entry is not None:
            self.entry[1].close()
            self.entry = None


def _ptr(t):
    return None if t is None else t.data_ptr()


def state_block(seed, it=0):
    """a `moca_fifo_state` (head 0, iteration `it`, the 64-bit seed, ext_noise 0) as the host int32 tensor the device block is written from"""
    st = _l.FifoState(0, it, seed & 0xffffffff, (seed >> 32) & 0xffffffff, 0)
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.int32)


class _StepEngine:
    """what the four one-graph engines share: a `_Plan` whose recorded UNet forward is wrapped into the engine's own launches, one
    enqueue per step on the plan's stream, accessors that wait for that stream before they copy"""

    def _bind(self, model, x):
        """the constructor preamble: the model's UNet, packed, and the device of the latents `x` -> (unet, device)"""
        self.unet = unet = model.model.diffusion_model
        self.device = x.device
        if unet._packed is None:
            unet._pack()
        return unet, x.device

    def _wrap_plan(self, pre, post):
        """a step = pre() + the UNet forward + post(), recorded and captured as one sequence"""
        self.plan.steps = [pre] + self.plan.steps + [post]

    @contextlib.contextmanager
    def _step(self):
        """`with self._step():` -- the body (host-given noise, uploads) is enqueued on the plan's stream, ordered after the current one;
        then one replay of the wrapped sequence.  Nothing is synchronised."""
        with self.plan._enqueue():
            yield
            self.plan._replay()
        self.n_iter += 1

    def _fix_noise(self, *pairs):
        """host-given draws: copy every (destination slice, tensor) and tell the Philox launch to leave the buffer alone (ext_noise)"""
        for dst, src in pairs:
            dst.copy_(src.reshape(-1).to(self.device, torch.float32))
        self.state[4:5].fill_(1)

    def sync_to(self, stream=None):
        (stream or torch.cuda.current_stream(self.device)).wait_stream(self.plan.stream)

    def _copy(self, t, shape=None):
        """a copy of an engine buffer as of the last enqueued step (None stays None)"""
        self.sync_to()
        return None if t is None else (t if shape is None else t.view(shape)).clone()

    def latents(self):
        return self._copy(self.plan.x_in)

    def close(self):
        self.plan.close()


class FifoEngine(_StepEngine):
    """Device-resident MoCA-FIFO loop, prompt mode and DAVIS-video mode.  `supported(...)` says whether a call can run here;
    `fifo.fifo_ddim_sampling` falls back to its host-driven loop otherwise (a mask-producer callback, per-call mask lists, a model
    that is not ours).

    DAVIS mode (`anchor_moments`): the FreeInit anchor of every shift is a fresh posterior sample of the VAE encoding of the LAST
    DAVIS frame (funcs.py:101-108) -- the frame never changes, so its moments [1, 2z, h, w] are encoded ONCE by the caller and an
    iteration only draws `scale_factor * (mean + std * noise)` (`moca_gaussian_sample_f32`) in front of the mix."""

    @staticmethod
    def supported(model, cond, latents, davis_data=None, sam_masks_fn=None):
        return (isinstance(unet_of(model), UNetModel) and isinstance(cond, dict) and "c_crossattn" in cond
                and (davis_data is None or getattr(model, "first_stage_model", None) is not None)
                and sam_masks_fn is None and latents is not None and latents.is_cuda and latents.shape[0] == 1)

    def __init__(self, args, model, sampler, cond, uc, cfg_scale, latents, conditioned_image=None, masks=None, gamma=0.5,
                 n_slots=1, seed=0, anchor_moments=None, scale_factor=1.0, sam_capacity=0):
        """sam_capacity > 0 (and no `masks`): prompt mode with precomputed Grounded-SAM-2 candidates -- `ddim_step`'s segmentation
        branch (ddim.py:592-606 -> `_apply_segmentation` :739-903) runs inside the iteration graph on at most `sam_capacity`
        candidate masks per iteration, handed to `step(sam_masks=...)`."""
        refuse_long_window(args)
        refuse_image_attention(model)
        refuse_concat(model, cond)
        unet, dev = self._bind(model, latents)
        f = args.video_length
        wins = list(fifo_windows(args))
        self.wins, self.nW, self.f = wins, len(wins), f
        nW = self.nW
        _, Cc, Q, H, W = latents.shape
        HW = H * W
        self.C, self.Q, self.H, self.W, self.HW = Cc, Q, H, W, HW
        self.lookahead = bool(args.lookahead_denoising)
        self.emit_frame = f // 2 if self.lookahead else 0
        guided = uc is not None and cfg_scale != 1.0
        self.reps = 2 if guided else 1
        # ---- timesteps / coefficient tables per window slot (funcs.py:290-294,311-312; ddim.py:405-430,565-582)
        timesteps, indices = lookahead_schedule(sampler, args)
        coef = np.zeros((nW, f, 6), np.float32)
        enh = np.ones((nW, f), np.float32)
        mframe = np.full((nW, f), -1, np.int32)
        t_rows = np.zeros((nW, f), np.int64)
        for w, (s0, _, e0) in enumerate(wins):
            t_rows[w] = timesteps[s0:e0]
            Fm = 0 if masks is None else max(0, min(e0, masks.shape[2]) - s0)
            coef[w], enh[w], mi = sampler.step_tables(indices[s0:e0], timesteps[s0:e0], H, Fm)
            mframe[w] = np.where(mi >= 0, s0 + mi, -1)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.coef, self.enh, self.mframe = to_dev(coef), to_dev(enh), to_dev(mframe)
        self.win_start = to_dev(np.asarray([s0 for s0, _, _ in wins], np.int32))
        # ---- the batched UNet plan: [conditional windows | unconditional windows], one context segment each
        ctxs = [context(c).expand(nW, -1, -1) for c in [cond] + ([uc] if guided else [])]
        segs = tuple((nW, int(c.shape[1])) for c in ctxs)
        B = self.reps * nW
        # guided: the unconditional windows are the SAME latents with another context: one plan whose prefix (everything before the
        # first cross-attention) runs once for both branches
        # (the prefix adds ONE fps embedding: branches with different fps run as a plain batch of 2 nW videos instead)
        fps_c = cond.get("fps", 16)
        shared = guided and same_fps([fps_c, uc.get("fps", fps_c)])
        self.gather_reps = 1 if shared or not guided else 2
        self.plan = plan = _Plan(unet, B, f, H, W, segs, torch.float32, dev, shared_x=shared)

        # (one fps per branch: of a tensor the first value serves all windows)
        fr = [fps_rows(one_fps(fp), nW, f, dev) for fp in [fps_c] + ([uc.get("fps", fps_c)] if guided else [])]
        with torch.cuda.stream(plan.stream):
            plan.t_rows.copy_(to_dev(t_rows).reshape(-1).repeat(self.reps))
            plan.fps_rows.copy_(torch.cat(fr))
            r = 0
            for c in ctxs:
                n = c.shape[0] * c.shape[1]
                plan.ctx[r:r + n].copy_(c.reshape(n, -1))
                r += n
        # ---- device state
        f32 = dict(dtype=torch.float32, device=dev)
        self.queue = latents[0].to(torch.float32).reshape(Cc, Q, HW).clone()
        self.state = state_block(seed).to(dev)
        n_win = nW * Cc * f * HW
        self.noise = torch.zeros(n_win + 2 * Cc * HW, **f32)         # [nW][C][f][HW] window noise | [C][HW] enqueued noise | [C][HW] anchor draw
        self.moments = None
        if anchor_moments is not None:
            self.moments = anchor_moments.to(dev, torch.float32).reshape(2 * Cc, HW).contiguous()
        self.momentum = torch.zeros(nW, Cc, f, HW, **f32)            # ddim.py:395-397
        self.pred_x0 = torch.empty(nW, Cc, f, HW, **f32)
        self.x_prev = torch.empty(nW, Cc, f, HW, **f32)
        self.anchor = torch.empty(Cc, HW, **f32)
        self.newframe = torch.empty(Cc, HW, **f32)
        self.n_slots = max(1, int(n_slots))
        self.emitted = torch.zeros(self.n_slots, Cc, HW, **f32)
        self.lpf = get_freq_filter((1, Cc, 1, H, W), dev, "gaussian", 1, 0.25, 0.25).reshape(-1, 1, H, W)[0].contiguous()   # funcs.py:95
        lib = _l.load()
        self.mix_ws = torch.empty(int(lib.moca_freq_mix_ws_bytes(Cc, 1, H, W)) // 4, **f32)
        self.mask = self.mask_sums = self.cond = None
        self.sam_capacity = int(sam_capacity) if masks is None else 0
        self._t_host = t_rows                                     # [nW][f] timesteps (host copy: which frames take the <= 300 branch)
        if self.sam_capacity > 0:
            self.sam_cand = torch.zeros(self.sam_capacity, HW, **f32)
            self.sam_tab = torch.zeros(2, nW * f, dtype=torch.int32, device=dev)          # [0] pool offset, [1] candidate count
            self.sam_eff = torch.zeros(nW, f, HW, **f32)
            self.sam_idx = torch.full((nW * f,), -1, dtype=torch.int32, device=dev)
            self._sam_stage = [(torch.empty(self.sam_capacity, HW, dtype=torch.float32).pin_memory(),
                                torch.zeros(2, nW * f, dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(2)]
            self._sam_turn = 0
            self.cond = cond_image_rows(conditioned_image, Cc, HW, dev)[0].contiguous()
        if masks is not None:
            if masks.shape[2] != Q:
                raise ValueError("the device-resident loop wants one mask frame per queue frame")
            self.mask = masks[0, 0].to(torch.float32).reshape(Q, HW).clone()
            self.mask_sums = torch.empty(Q, **f32)
            _l.check(lib.moca_mask_frame_sums_f32(_l.ptr(self.mask), _l.ptr(self.mask_sums), Q, HW,
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "moca_mask_frame_sums_f32")
            self.cond = cond_image_rows(conditioned_image, Cc, HW, dev)[0].contiguous()
        torch.cuda.current_stream(dev).synchronize()
        # ---- the launch sequence of one iteration = [noise, gather] + UNet + [guidance + step + write-back, FreeInit mix, advance]
        p = _l.FifoStepParams()
        p.state, p.x = self.state.data_ptr(), plan.x_in.data_ptr()
        eps = plan.out.reshape(B, -1)
        p.eps_c = eps[:nW].data_ptr()
        p.eps_u = eps[nW:].data_ptr() if guided else None
        p.noise, p.momentum, p.queue = self.noise.data_ptr(), self.momentum.data_ptr(), self.queue.data_ptr()
        p.x_prev, p.pred_x0 = self.x_prev.data_ptr(), self.pred_x0.data_ptr()
        p.coef, p.win_start = self.coef.data_ptr(), self.win_start.data_ptr()
        p.mask, p.mask_sums = _ptr(self.mask), _ptr(self.mask_sums)
        p.mask_frame, p.enh, p.cond = self.mframe.data_ptr(), self.enh.data_ptr(), _ptr(self.cond)
        if self.sam_capacity > 0:
            p.sam_eff, p.sam_idx = self.sam_eff.data_ptr(), self.sam_idx.data_ptr()
        p.cfg_scale = float(cfg_scale)
        p.beta, p.one_minus_beta = float(np.float32(sampler.beta)), float(np.float32(1 - sampler.beta))
        p.gamma, p.one_minus_gamma = float(np.float32(gamma)), float(np.float32(1 - gamma))
        p.nW, p.C, p.Q, p.f, p.HW = nW, Cc, Q, f, HW
        p.wb_from = f // 2 if self.lookahead else 0
        self._params = p
        st_, q_ = _l.ptr(self.state), _l.ptr(self.queue)
        S = lambda: C.c_void_p(ops.current_stream())

        def pre():
            _l.check(lib.moca_fifo_randn_f32(st_, _l.ptr(self.noise), self.noise.numel(), S()), "moca_fifo_randn_f32")
            # the FreeInit anchor is frame 0 AFTER the write-backs (funcs.py:88): only with lookahead is it untouched by them
            early_anchor = self.moments is None and self.lookahead
            _l.check(lib.moca_fifo_gather_windows_f32(st_, q_, _l.ptr(plan.x_in), _l.ptr(self.anchor) if early_anchor else None,
                                                      _l.ptr(self.win_start), nW, self.gather_reps, Cc, Q, f, HW, S()), "moca_fifo_gather_windows_f32")

        def post():
            if self.sam_capacity > 0:      # which candidate masks each window frame injects (pre_masks / IoU / > 80 % bookkeeping)
                _l.check(lib.moca_sam_select_masks_f32(_l.ptr(self.sam_cand), _l.ptr(self.sam_tab[0]), _l.ptr(self.sam_tab[1]),
                                                       _l.ptr(plan.t_rows), _l.ptr(self.sam_eff), _l.ptr(self.sam_idx), nW, f, HW, S()),
                         "moca_sam_select_masks_f32")
            _l.check(lib.moca_fifo_step_windows_f32(C.byref(p), S()), "moca_fifo_step_windows_f32")
            if self.moments is None and not self.lookahead:  # rank 0 rewrote frame 0 (funcs.py:353-354): read the anchor now
                _l.check(lib.moca_fifo_gather_windows_f32(st_, q_, None, _l.ptr(self.anchor), None, 0, 1, Cc, Q, f, HW, S()),
                         "moca_fifo_gather_windows_f32")
            if self.moments is not None:                     # anchor = get_first_stage_encoding(posterior of the last DAVIS frame) (:108)
                _l.check(lib.moca_gaussian_sample_f32(_l.ptr(self.moments), _l.ptr(self.noise[n_win + Cc * HW:]), _l.ptr(self.anchor), 1, Cc, HW,
                                                      float(scale_factor), S()), "moca_gaussian_sample_f32")
            _l.check(lib.moca_freq_mix_3d_f32(_l.ptr(self.anchor), _l.ptr(self.noise[n_win:n_win + Cc * HW]), _l.ptr(self.lpf), _l.ptr(self.newframe),
                                              Cc, 1, H, W, _l.ptr(self.mix_ws), S()), "moca_freq_mix_3d_f32")
            _l.check(lib.moca_fifo_advance_f32(st_, q_, _l.ptr(self.newframe), _l.ptr(self.emitted), self.n_slots, self.emit_frame,
                                               _l.ptr(self.mask), _l.ptr(self.mask_sums), Cc, Q, HW, S()), "moca_fifo_advance_f32")
        self.n_unet_launches = len(plan.steps)
        self._wrap_plan(pre, post)
        self.n_iter = 0
        sampler.momentum = self.momentum[nW - 1].view(1, Cc, f, H, W)      # what the reference's last call (rank 0) leaves behind

    def _upload_sam(self, sam_masks):
        """pack the candidates of this iteration -- `sam_masks[w][i]` = [n,H,W] masks Grounded-SAM-2 returns for frame i of window w
        (reference call order), None / empty = no box -- into the pool and enqueue the copy on the plan's stream.  Frames with
        t > 300 never reach the producer (ddim.py:592) and are not uploaded.  Host tensors go through a pinned double buffer (no
        host synchronisation unless the copy of two iterations ago is still in flight); tensors already on the device are copied
        there (stream-ordered, nothing read back: only their shapes are looked at)."""
        pool, tab, ev = self._sam_stage[self._sam_turn]
        self._sam_turn ^= 1
        ev.synchronize()
        tab.zero_()
        used, host_runs, dev_copies = 0, [], []
        if sam_masks is not None:
            for w in range(self.nW):
                cw = sam_masks[w]
                for i in range(self.f):
                    if self._t_host[w, i] > 300 or cw is None or i >= len(cw) or cw[i] is None:
                        continue
                    m = torch.as_tensor(cw[i]).detach().reshape(-1, self.HW)
                    n = m.shape[0]
                    if n == 0:
                        continue
                    if used + n > self.sam_capacity:
                        raise ValueError(f"more than sam_capacity = {self.sam_capacity} candidate masks in one iteration")
                    if m.is_cuda:
                        dev_copies.append((used, n, m))
                    else:
                        pool[used:used + n].copy_(m.to(torch.float32))
                        host_runs.append((used, n))
                    tab[0, w * self.f + i], tab[1, w * self.f + i] = used, n
                    used += n
        for a, n in host_runs:
            self.sam_cand[a:a + n].copy_(pool[a:a + n], non_blocking=True)
        for a, n, m in dev_copies:
            self.sam_cand[a:a + n].copy_(m.to(self.device, torch.float32), non_blocking=True)
        self.sam_tab.copy_(tab, non_blocking=True)
        ev.record(self.plan.stream)

    def set_context(self, cond_ctx):
        """The prompt switch of funcs.py:426-430: replace the conditional windows' context rows of `plan.ctx` between two iterations.
        `cond_ctx` [1,L,D] (or a `c_crossattn` list, concatenated as the constructor does) must have the token count L the plan was
        built with.  The copy is enqueued on the plan's stream, after the iteration enqueued last and before the next one, whose
        in-graph K|V projection (`_Plan.kv_all`, a recorded step) reads it; nothing else of the plan is derived from the context, so
        no plan is rebuilt and no graph re-captured.  The unconditional rows, the queue and the device state stay as they are."""
        c = torch.cat(list(cond_ctx), 1) if isinstance(cond_ctx, (list, tuple)) else cond_ctx
        L = self.plan.segs[0][1]
        if c.dim() != 3 or c.shape[0] != 1 or c.shape[1] != L:
            raise ValueError(f"set_context: the plan's conditional segment holds [1, {L}, D] contexts, got {tuple(c.shape)}")
        plan = self.plan
        src = c.to(self.device)
        with plan._enqueue():
            plan.set_context([src.expand(self.nW, -1, -1)])       # (only the first segment: zip over the plan's segments)
        src.record_stream(plan.stream)

    # ------------------------------------------------------------------------------------------------------------------
    def step(self, noise=None, shift_noise=None, anchor_noise=None, sam_masks=None):
        """one outer iteration (enqueued, not synchronised).  `noise` = list over windows (reference order: rank 2n-1 .. 0) of
        [1,C,f,H,W] tensors, `shift_noise` [1,C,H,W] and (DAVIS mode) `anchor_noise` [1,C,1,H,W] fix the draws (all or none);
        `sam_masks` (engines built with sam_capacity): this iteration's candidate masks, see `_upload_sam`."""
        with self._step():
            if self.sam_capacity > 0:
                self._upload_sam(sam_masks)
            elif sam_masks is not None:
                raise ValueError("this engine was built without sam_capacity")
            if noise is not None:
                n_win, chw = self.nW * self.C * self.f * self.HW, self.C * self.HW
                self._fix_noise((self.noise[:n_win], torch.stack([n.reshape(-1) for n in noise])),
                                (self.noise[n_win:n_win + chw], shift_noise),
                                *([(self.noise[n_win + chw:], anchor_noise)] if anchor_noise is not None else []))   # (the advance clears ext_noise)

    def latents(self):
        """the queue in frame order [1,C,Q,H,W] (a copy; the ring itself never moves)"""
        self.sync_to()
        head = self.n_iter % self.Q
        return torch.roll(self.queue, -head, dims=1).reshape(1, self.C, self.Q, self.H, self.W)

    def mask_queue(self):
        self.sync_to()
        head = self.n_iter % self.Q
        return None if self.mask is None else torch.roll(self.mask, -head, dims=0).reshape(1, 1, self.Q, self.H, self.W)

    def emitted_frames(self, i0, i1):
        """latent frames emitted by iterations i0 .. i1-1 as [1,C,i1-i0,H,W] (they must still be in the slot ring)"""
        self.sync_to()
        assert self.n_iter - i0 <= self.n_slots and i1 <= self.n_iter
        idx = [i % self.n_slots for i in range(i0, i1)]
        return self.emitted[idx].permute(1, 0, 2).reshape(1, self.C, len(idx), self.H, self.W)

    def window_outputs(self):
        """(x_prev, pred_x0) of the last iteration's windows, [nW][1,C,f,H,W] views in the reference's call order"""
        self.sync_to()
        v = lambda t: [t[w].view(1, self.C, self.f, self.H, self.W) for w in range(self.nW)]
        return v(self.x_prev), v(self.pred_x0)


class _TrajectoryEngine(_StepEngine):
    """What `BaseEngine`, `InvertEngine` and `DdpmEngine` share: B latents that live in the plan's input buffer and take one sampler
    step per replay, the step's schedule row picked by the state block's iteration counter (row S - 1 - iter of `t_table` and of the
    engine's coefficient table).  With guidance the plan holds 2 B rows -- the conditional and the unconditional branch of the SAME
    latents, one context segment each, everything before the first cross-attention computed once (`shared_x`) -- else B rows and one
    segment.  A subclass adds its tables and buffers, the step kernel (`_wrap_step`) and what its `reset` writes beside the core
    (`_restart`)."""
    pred_x0 = None

    @staticmethod
    def _supports(model, x, branches):
        """the clauses every `supported()` starts with: our UNet, latents on the device, every branch a dict with the conditional
        branch's keys, at most 64 rows in the plan"""
        return (isinstance(unet_of(model), UNetModel) and x.is_cuda and all(isinstance(c, dict) for c in branches)
                and all(set(c.keys()) == set(branches[0].keys()) for c in branches[1:]) and len(branches) * x.shape[0] <= 64)

    @staticmethod
    def _supports_crossattn(model, branches):
        """'crossattn' models with `c_crossattn` / `fps` conditioning only, one fps for all branches (the shared prefix adds ONE fps
        embedding)"""
        return (conditioning_key(model) == "crossattn" and set(branches[0].keys()) <= {"c_crossattn", "fps"}
                and same_fps([c.get("fps", 16) for c in branches]))

    def _open(self, model, x, branches, S, pieces=None, features_adapter=None):
        """the head of every constructor: the preamble, the plan for `branches` ([cond] or [cond, uc]) -- with the `c_concat` channel
        counts `pieces` and buffers for the `features_adapter` maps where given -- and the state block -> (device, elements of x)"""
        unet, dev = self._bind(model, x)
        unet._check_adapter(features_adapter)                # (the list length fails as in UNetModel.forward)
        B, _, T, H, W = self.shape = tuple(x.shape)
        self.S, self.guided = S, len(branches) == 2
        L = tuple((B, n_ctx(c)) for c in branches) if self.guided else n_ctx(branches[0])
        self.plan = _Plan(unet, len(branches) * B, T, H, W, L, torch.float32, dev, shared_x=self.guided, pieces=pieces,
                          adapter=None if features_adapter is None else unet.adapter_sites)
        self.state = torch.zeros(8, dtype=torch.int32, device=dev)
        return dev, x.numel()

    def _blend_launch(self):
        """None, or `blend(lib, state, stream)`: what a masked engine launches on the latents in front of the forward"""
        return None

    def _wrap_step(self, draw, step):
        """the launch sequence of one replay: [timestep rows of table row S - 1 - iter; the Philox draws over the buffer `draw`, None:
        nothing is drawn; on a masked engine the blend of `_blend_launch`, behind the draw] + the UNet forward + [`step(lib, state,
        eps_c, eps_u, stream)`: the engine's step kernel on the conditional rows of `plan.out` and the unconditional ones, NULL without
        guidance]"""
        lib, plan, B = _l.load(), self.plan, self.shape[0]
        blend = self._blend_launch()
        eps = plan.out.reshape((2 if self.guided else 1) * B, -1)
        st_ = _l.ptr(self.state)
        S_ = lambda: C.c_void_p(ops.current_stream())

        def pre():
            _l.check(lib.moca_base_set_timestep(st_, _l.ptr(self.t_table), self.S, _l.ptr(plan.t_rows), plan.t_rows.numel(), S_()), "moca_base_set_timestep")
            if draw is not None:
                _l.check(lib.moca_fifo_randn_f32(st_, _l.ptr(draw), draw.numel(), S_()), "moca_fifo_randn_f32")
            if blend is not None:
                blend(lib, st_, S_())

        def post():
            step(lib, st_, _l.ptr(eps[:B]), _l.ptr(eps[B:]) if self.guided else None, S_())
        self._wrap_plan(pre, post)

    def _wrap_ddim_step(self, draw, noise, cfg_scale, use_scale):
        """`_wrap_step` with `moca_base_ddim_step_f32`, in place on the plan's input buffer, `noise` its noise operand"""
        plan, n = self.plan, noise.numel()
        self._wrap_step(draw, lambda lib, st_, eps_c, eps_u, stream: _l.check(lib.moca_base_ddim_step_f32(
            st_, _l.ptr(plan.x_in), eps_c, eps_u, _l.ptr(noise), _l.ptr(self.pred_x0), _l.ptr(self.coef), self.S, float(cfg_scale),
            1 if use_scale else 0, n, stream), "moca_base_ddim_step_f32"))

    def _refuse_other_shape(self, x):
        if tuple(x.shape) != self.shape:
            raise ValueError(f"x {tuple(x.shape)} does not match the engine's latents {self.shape}")

    @contextlib.contextmanager
    def _restart(self, x, cond, uc, seed=0, fps=None):
        """the core of every `reset`, `with self._restart(...):` -- a new trajectory on the same plan and the same captured graph: the
        state block (iteration 0, the noise stream of `seed`), the latents `x`, the fps rows and the context of every branch (`fps`:
        one per branch, default the branches' own), all enqueued on the plan's stream; the body, what the engine adds, is enqueued
        behind them; then the current stream waits for the plan's"""
        plan, dev = self.plan, self.device
        B, T = self.shape[0], self.shape[2]
        branches = [cond, uc] if self.guided else [cond]
        fps = [c.get("fps", 16) for c in branches] if fps is None else fps
        if not same_fps(fps):
            raise ValueError(f"{type(self).__name__} shares the UNet prefix between the two guidance branches: their fps must be equal")
        ctxs = [context(c).expand(B, -1, -1) for c in branches]
        with plan._enqueue():
            self.state.copy_(state_block(seed))
            plan.x_in.copy_(x.to(torch.float32))
            plan.fps_rows.copy_(torch.cat([fps_rows(fp, B, T, dev) for fp in fps]))
            plan.set_context(ctxs)
            yield
        self.sync_to()
        self.n_iter = 0

    def t_rows(self):
        """the timestep rows the UNet of the last step was given (a copy)"""
        return self._copy(self.plan.t_rows)

    def last_pred_x0(self):
        return self._copy(self.pred_x0, self.shape)


class BaseEngine(_TrajectoryEngine):
    """One step of base sampling -- `DDIMSampler.ddim_sampling`'s loop body (ddim.py:226-252: two UNet calls on the same latents, guidance,
    the DDIM update with `use_scale`, fresh noise) -- as ONE hipGraph: [timestep rows of step i, noise] + the shared-prefix UNet forward
    of the B latents x (conditional, unconditional) + [guidance + update in place, i += 1].  The latents live in the plan's input
    buffer, the schedule in device tables indexed by the state block's iteration counter; the host only replays.

    `n_rows` (default: the whole schedule) builds the tables over the FIRST n_rows schedule rows, so that the S of the captured kernels
    is n_rows and step i uses row n_rows - 1 - i: `DDIMSampler.decode(x, c, t_start)` (ddim.py:674-692) is this engine with
    n_rows = t_start.  `encode` noises a clean latent into the plan's input buffer (`stochastic_encode`, ddim.py:652-671) with the
    tables of the WHOLE schedule, so a video-to-video run is reset -> encode(x0, t_start) -> t_start steps, all on the device.

    `mask=` / `x0=` build a MASKED engine (inpainting, upstream's DDIM loop): in front of the forward of every step, behind the draws,
    `moca_ddpm_step_f32` in its blend-only mode (no eps) rewrites the latents in place, x = q_sample(x0, t_row) mask + (1 - mask) x:
    the kernel gathers the model's own q_sample tables at the plan's timestep rows, which the launch before it wrote, so the blend
    follows `n_rows` and `set_schedule` by itself.  Fresh q-noise every step: the step's Philox launch covers
    [noise | pad to 16 B | noise_q], as `DdpmEngine`'s.  `mask` and `x0` live on the device, written by `reset`.  Nothing is blended
    behind the last step.  An unmasked engine records exactly the launches it recorded before there was a mask."""

    @staticmethod
    def supported(model, x, cond, uc, scale, features_adapter=None):
        unet, key = unet_of(model), conditioning_key(model)
        if features_adapter is not None and key != "crossattn":
            return False                                     # (the host-issued path's wrapper names the refusal)
        if scale == 1.0 or not _TrajectoryEngine._supports(model, x, [cond, uc]):
            return False
        if key in ("hybrid", "hybrid-adm-mask"):
            # (the other hybrid keys need c_adm / s: they stay on the host-issued path, which keeps the reference's asserts.)  Both
            # guidance branches must see the SAME c_concat (funcs.py:211-214 copies cond and replaces c_crossattn only): the shared
            # prefix holds one set of input rows.  fps is dropped by these keys (ddpm3d.py:717), so nothing to compare
            a, b = cond.get("c_concat"), uc.get("c_concat")
            if a is None and key == "hybrid":
                return False
            # a wrong channel total goes to the host-issued path, whose wrapper names it in a ValueError
            if x.shape[1] + sum(int(c.shape[1]) for c in a or ()) != unet.in_channels:
                return False
            same = a is b or (a is not None and b is not None and len(a) == len(b) and all(
                p is q or (p.data_ptr() == q.data_ptr() and p.shape == q.shape and p.stride() == q.stride() and p.dtype == q.dtype)
                for p, q in zip(a, b)))
            return same and set(cond.keys()) <= {"c_crossattn", "fps", "c_concat"}
        return _TrajectoryEngine._supports_crossattn(model, [cond, uc])

    @staticmethod
    def key(sampler, x, cond, uc, cfg_scale, features_adapter=None, n_rows=None, mask=None):
        """what an engine built by `BaseEngine(model, sampler, x, cond, uc, cfg_scale, ...)` is good for: everything the plan and the
        captured launches bake in -- latent shape, context lengths, scale, the schedule's timesteps and sigmas, device, `c_concat`
        channel counts, adapter map shapes, the table rows (`n_rows` keeps `decode`'s engine and `sample`'s apart) and whether and how
        a mask is read (`mask_kind`, None without one)"""
        return (tuple(x.shape), n_ctx(cond), n_ctx(uc), float(cfg_scale), sampler.ddim_timesteps.tobytes(),
                np.asarray(sampler.ddim_sigmas).tobytes(), str(x.device), tuple(int(c.shape[1]) for c in cond.get("c_concat") or ()),
                None if features_adapter is None else tuple(tuple(f.shape) for f in features_adapter),
                len(sampler.ddim_timesteps) if n_rows is None else int(n_rows), None if mask is None else mask_kind(mask, x.shape))

    def __init__(self, model, sampler, x, cond, uc, cfg_scale, seed=0, keep_pred_x0=False, features_adapter=None, n_rows=None, mask=None,
                 x0=None):
        S = len(sampler.ddim_timesteps) if n_rows is None else int(n_rows)
        if not 1 <= S <= len(sampler.ddim_timesteps):
            raise ValueError(f"n_rows = {n_rows}: the schedule has {len(sampler.ddim_timesteps)} rows")
        # hybrid keys: x carries the latent channels only; the c_concat columns of the first conv's input rows are constant over a
        # trajectory (reset() writes them), the recorded step rewrites the latent columns from plan.x_in; fps is dropped (16).
        # features_adapter: constant over a trajectory like c_concat -- reset() writes the plan's adapter buffers, the recorded step
        # reads them
        self.hybrid = conditioning_key(model) != "crossattn"
        concat = cond.get("c_concat") if self.hybrid else None
        dev, n = self._open(model, x, [cond, uc], S, None if concat is None else tuple(int(c.shape[1]) for c in concat), features_adapter)
        self._built = self._schedule_tables(sampler, S)      # host copies: `reset` puts them back after a `set_schedule`
        self.coef, self.t_table = (t.to(dev) for t in self._built)
        self.it0, self._schedule_set = 0, False              # where a trajectory's iteration counter starts (`set_schedule`)
        self.enc_coef = self._built_enc = tuple(c.to(dev) for c in sampler.encode_tables())     # `encode`: the whole schedule's q_sample tables
        self.enc_state = torch.zeros(8, dtype=torch.int32, device=dev)        # the noise stream of `encode`: same seed, iteration -1
        self.model = model
        self._reinit_bufs = None                             # `reinit` (FreeInit): made by its first call
        self._reinit_src = (None, None)
        self._open_mask(x, mask, x0)
        n_pad = (n + 3) // 4 * 4                             # q_sample's draw starts 16-byte aligned
        draw = torch.zeros(n_pad + n if self.masked else n, dtype=torch.float32, device=dev)
        self.noise = draw[:n]                                # (what `encode` and `reinit` draw into, too)
        self.noise_q = draw[n_pad:] if self.masked else None
        self.pred_x0 = torch.empty(n, dtype=torch.float32, device=dev) if keep_pred_x0 else None
        self.reset(x, cond, uc, seed, features_adapter=features_adapter, mask=mask, x0=x0)
        self._wrap_ddim_step(draw, self.noise, cfg_scale, bool(sampler.use_scale))

    def _open_mask(self, x, mask, x0):
        """(constructor) the buffers of a masked engine: the mask as the kernel reads it and x0, both filled by `reset`; the blend reads
        the model's DDPM table (`sqrt_alphas_cumprod`, `sqrt_one_minus_alphas_cumprod`, `scale_arr` per timestep)"""
        if (mask is None) != (x0 is None):
            raise ValueError("mask= and x0= go together: the mask says where x0 is kept")
        self.masked = mask is not None
        self.mask = self.x0 = None
        self.mask_inner = self.blend_flags = 0
        if self.masked:
            m, mflag, self.mask_inner = mask_operand(mask, x.shape, self.device)
            self.blend_flags = mflag | self.model._ddpm_flags(x0_param=False)
            self.mask = torch.empty_like(m)
            self.x0 = torch.empty(x.numel(), dtype=torch.float32, device=self.device)
            self.blend_coef = self.model._ddpm_dev(self.device)["coef"]

    def _blend_launch(self):
        if not self.masked:
            return None
        plan, (B, T), n = self.plan, (self.shape[0], self.shape[2]), self.x0.numel()
        # (state NULL: the counter is the step kernel's to advance; t = the timestep rows, row stride = frames, as DdpmEngine reads them)
        return lambda lib, st_, stream: _l.check(lib.moca_ddpm_step_f32(
            None, _l.ptr(plan.x_in), _l.ptr(plan.x_in), None, None, None, None, None, _l.ptr(self.mask), _l.ptr(self.x0), _l.ptr(self.noise_q),
            _l.ptr(self.blend_coef), _l.ptr(plan.t_rows), T, B, int(self.blend_coef.shape[0]), n // B, self.mask_inner, 1.0, 1.0,
            self.blend_flags, stream), "moca_ddpm_step_f32")

    def _checked_mask(self, mask, x0):
        """(`reset`, before anything is enqueued) `DdpmEngine.reset`'s validation -> the mask as the kernel reads it, None unmasked"""
        if (mask is not None) != self.masked or (x0 is not None) != self.masked:
            raise ValueError("mask and x0 go with an engine built for them")
        if not self.masked:
            return None
        m, _, inner = mask_operand(mask, self.shape, self.device)
        if m.shape != self.mask.shape or inner != self.mask_inner:
            raise ValueError(f"mask {tuple(mask.shape)} is read another way than the mask the engine was built with")
        if tuple(x0.shape) != self.shape:
            raise ValueError(f"x0 {tuple(x0.shape)} does not match the engine's latents {self.shape}")
        return m

    @staticmethod
    def _schedule_tables(sampler, n_rows):
        """host tables over the first `n_rows` rows of the sampler's schedule: coef [n_rows][8] = {the five of ddim_coef, scale,
        scale_prev (1 without use_scale), unused} and the int64 timesteps"""
        coef = np.zeros((n_rows, 8), np.float32)
        use_scale = bool(sampler.use_scale)
        for i in range(n_rows):
            coef[i, :5] = ddim_coef(sampler, i)
            coef[i, 5:7] = (sampler.ddim_scale_arr[i], sampler.ddim_scale_arr_prev[i]) if use_scale else 1.0
        t_table = np.ascontiguousarray(np.asarray(sampler.ddim_timesteps, dtype=np.int64)[:n_rows])
        return torch.from_numpy(coef), torch.from_numpy(t_table)

    def _write_schedule(self, coef, t_table):
        """(inside an enqueue) the tables into rows 0 .. len-1 of the device tables, the start of the iteration counter moved so that
        step i of a trajectory reads row len - 1 - i through the captured S (row S - 1 - iter)"""
        n = int(t_table.shape[0])
        self.coef[:n].copy_(coef)
        self.t_table[:n].copy_(t_table)
        self.state[1:2].fill_(self.S - n)
        self.it0 = self.n_iter = self.S - n

    def set_schedule(self, sampler):
        """Run the next trajectories over `sampler`'s current schedule of S' <= S steps WITHOUT a new capture (FreeInit's coarse-to-fine
        iterations).  S is a launch argument baked into the captured `moca_base_set_timestep` / `moca_base_ddim_step_f32`, which read
        table row S - 1 - iter: the S' rows of the new schedule go to rows 0 .. S'-1 of the device tables and the iteration counter
        starts at S - S', so step i reads row S' - 1 - i.  The graph, the plan and its buffers are untouched; `encode` follows the
        new schedule.  Enqueued, not synchronised; holds until the next `set_schedule` or `reset` (which puts the engine's own schedule
        back).  Call it between trajectories: it sets the counter to the start of one."""
        n = len(sampler.ddim_timesteps)
        if not 1 <= n <= self.S:
            raise ValueError(f"set_schedule: a schedule of {n} steps does not fit the {self.S} rows this engine was captured for")
        with self.plan._enqueue():
            self._write_schedule(*self._schedule_tables(sampler, n))
        self.enc_coef = tuple(c.to(self.device) for c in sampler.encode_tables())
        self._schedule_set = True

    def reinit(self, initial_noise, lpf, z_rand=None, seed=0):
        """FreeInit's noise re-initialisation of the latents in the plan's input buffer (`freeinit.freeinit_reinit` on the device), on
        the plan's stream, enqueued and not synchronised: x_in <- freq_mix_3d(q_sample(x_in, t = num_timesteps - 1, initial_noise),
        z_rand, lpf) with the model's DDPM tables (`moca_ddpm_step_f32` in its q_sample mode: `use_scale` multiplies by scale_arr[t]),
        then the state block back to the start of a trajectory with the new `seed`.  `z_rand` None: drawn by `moca_fifo_randn_f32` from
        the engine's own Philox stream (the new seed at iteration -2, which neither a step nor `encode` uses).  `initial_noise` and the
        filter volume `lpf` ([..., T, H, W], constant over the leading dims) are written to the device once per run: again only when
        another tensor object is handed in, or after `reset`.  Contexts, fps rows, adapter maps and c_concat columns are not touched."""
        plan, dev = self.plan, self.device
        B, Cc, T, H, W = self.shape
        n = self.noise.numel()
        lib = _l.load()
        model = self.model
        if self._reinit_bufs is None:
            f32 = dict(dtype=torch.float32, device=dev)
            self._reinit_bufs = dict(
                coef=model._ddpm_dev(dev)["coef"], flags=model._ddpm_flags(x0_param=False),
                t_last=torch.full((B,), model.num_timesteps - 1, dtype=torch.int64, device=dev),
                state=torch.zeros(8, dtype=torch.int32, device=dev), init_noise=torch.empty(n, **f32), lpf=torch.empty(T * H * W, **f32),
                z_T=torch.empty(n, **f32), ws=torch.empty(int(lib.moca_freq_mix_ws_bytes(B * Cc, T, H, W)) // 4, **f32))
        b = self._reinit_bufs
        if tuple(initial_noise.shape) != tuple(self.shape):
            raise ValueError(f"initial_noise {tuple(initial_noise.shape)} does not match the engine's latents {tuple(self.shape)}")
        if tuple(lpf.shape[-3:]) != (T, H, W):
            raise ValueError(f"lpf {tuple(lpf.shape)} is no filter over the engine's (T, H, W) = {(T, H, W)}")
        if z_rand is not None and z_rand.numel() != n:
            raise ValueError(f"z_rand {tuple(z_rand.shape)} does not match the engine's latents {tuple(self.shape)}")
        with plan._enqueue():
            h = C.c_void_p(plan.stream.cuda_stream)
            def upload(dst, src):
                src = src.to(dev, torch.float32)
                dst.copy_(src.reshape(-1), non_blocking=True)
                src.record_stream(plan.stream)
            if self._reinit_src[0] is not initial_noise:
                upload(b["init_noise"], initial_noise)
            if self._reinit_src[1] is not lpf:
                upload(b["lpf"], lpf[(0,) * (lpf.dim() - 3)])
            self._reinit_src = (initial_noise, lpf)
            _l.check(lib.moca_ddpm_step_f32(None, None, _l.ptr(b["z_T"]), None, None, None, None, None, None, _l.ptr(plan.x_in),
                                            _l.ptr(b["init_noise"]), _l.ptr(b["coef"]), _l.ptr(b["t_last"]), 1, B, int(b["coef"].shape[0]),
                                            n // B, 0, 1.0, 1.0, b["flags"], h), "moca_ddpm_step_f32")
            if z_rand is not None:
                upload(self.noise, z_rand)
            else:
                self._fill_state(b["state"], seed, -2)
                _l.check(lib.moca_fifo_randn_f32(_l.ptr(b["state"]), _l.ptr(self.noise), n, h), "moca_fifo_randn_f32")
            _l.check(lib.moca_freq_mix_3d_f32(_l.ptr(b["z_T"]), _l.ptr(self.noise), _l.ptr(b["lpf"]), _l.ptr(plan.x_in), B * Cc, T, H, W,
                                              _l.ptr(b["ws"]), h), "moca_freq_mix_3d_f32")
            self._fill_state(self.state, seed, self.it0)
            self._fill_state(self.enc_state, seed, -1)
        self.n_iter = self.it0

    @staticmethod
    def _fill_state(st, seed, it):
        """`state_block(seed, it)` into the device block `st` by fills on the current stream: no host buffer, nothing to wait for"""
        for i, v in enumerate((0, it, seed & 0xffffffff, (seed >> 32) & 0xffffffff, 0)):
            st[i:i + 1].fill_(v - (1 << 32) if v >= 1 << 31 else v)

    def reset(self, x, cond, uc, seed=0, features_adapter=None, mask=None, x0=None):
        """start a new trajectory on the same plan: latents x_T, contexts, fps, adapter maps, iteration 0, a new noise stream; on a
        masked engine `mask` (read the way the engine's mask is) and `x0`; the engine's own schedule, should `set_schedule` have
        replaced it"""
        plan = self.plan
        if (features_adapter is None) != (plan.adapter_in is None):
            raise ValueError("features_adapter goes with an engine built for it")
        m = self._checked_mask(mask, x0)
        with self._restart(x, cond, uc, seed, fps=(16, 16) if self.hybrid else None):
            if m is not None:
                self.mask.copy_(m)
                self.x0.copy_(x0.reshape(-1).to(self.device, torch.float32))
            if self._schedule_set:                               # (the built tables end at row S - 1: the counter stays at 0)
                self._write_schedule(*self._built)
                self.enc_coef, self._schedule_set = self._built_enc, False
            self._reinit_src = (None, None)
            self.enc_state.copy_(state_block(seed, -1))          # (no step ever draws at this iteration: steps count up from 0)
            if features_adapter is not None:
                plan.set_adapter(list(features_adapter))
            if plan.pieces is not None:
                with plan._ops_stream():
                    plan.set_concat(cond["c_concat"])

    def encode(self, x0, t_index, noise=None):
        """`stochastic_encode` (ddim.py:652-671) into the plan's input buffer: x_in = sqrt(a)[t] x0 + sqrt(1 - a)[t] noise on the plan's
        stream (enqueued, not synchronised), the start of a video-to-video trajectory.  `t_index`: one schedule index for all samples or
        a [B] tensor of them, on either device (host values are range-checked; the kernel gathers).  `noise` None: drawn by
        `moca_fifo_randn_f32` from the engine's own Philox stream (this trajectory's seed at iteration -1, which no step uses), so
        nothing moves through the host."""
        plan, dev = self.plan, self.device
        B = self.shape[0]
        if tuple(x0.shape) != tuple(self.shape):
            raise ValueError(f"x0 {tuple(x0.shape)} does not match the engine's latents {tuple(self.shape)}")
        t = torch.as_tensor(t_index)
        n_tab = int(self.enc_coef[0].shape[0])
        t = check_schedule_index(t.reshape(1).expand(B) if t.dim() == 0 else t, B, n_tab)
        lib = _l.load()
        n = self.noise.numel()
        with plan._enqueue():
            h = C.c_void_p(plan.stream.cuda_stream)
            src = x0.to(dev, torch.float32).contiguous()
            t_d = t.to(dev, torch.int64).contiguous()
            if noise is not None:
                self.noise.copy_(noise.reshape(-1).to(dev, torch.float32))
            else:
                _l.check(lib.moca_fifo_randn_f32(_l.ptr(self.enc_state), _l.ptr(self.noise), n, h), "moca_fifo_randn_f32")
            _l.check(lib.moca_q_sample_f32(_l.ptr(src), _l.ptr(self.noise), _l.ptr(plan.x_in), _l.ptr(self.enc_coef[0]), _l.ptr(self.enc_coef[1]),
                                           _l.ptr(t_d), B, n_tab, n // B, h), "moca_q_sample_f32")
        src.record_stream(plan.stream)
        t_d.record_stream(plan.stream)

    def step(self, noise=None, mask_noise=None):
        """one DDIM step (enqueued, not synchronised); `noise` [B,C,T,H,W] fixes the draw and, on a masked engine, `mask_noise`
        q_sample's (both or neither: one flag tells the Philox launch that the host filled the buffer)"""
        if (mask_noise is not None) != (self.masked and noise is not None):
            raise ValueError("a masked engine takes the step's two draws together, noise and mask_noise, or neither; an unmasked one "
                             "has no mask_noise")
        with self._step():
            if noise is not None:
                self._fix_noise((self.noise, noise), *([(self.noise_q, mask_noise)] if self.masked else []))


class DpmEngine(BaseEngine):
    """One step of DPM-Solver++(2M) sampling (`DPMSolverSampler`) as ONE hipGraph: `BaseEngine`'s two launches around the forward,
    `moca_base_set_timestep` and `moca_base_ddim_step_f32`, the latter with MOCA_BASE_MULTISTEP in its flag word and on the tables of
    `dpmpp_tables`.  `reset`, `encode`, `reinit`, `set_schedule`, `n_rows`, `c_concat` and `features_adapter` are `BaseEngine`'s.  What
    differs:

      * nothing is drawn in a step: no `moca_fifo_randn_f32` launch, `step()` takes no noise.  The step kernel's noise operand (not
        read) is the buffer `encode` and `reinit` draw into.  The one exception is a MASKED engine (`mask=` / `x0=`, as `BaseEngine`'s):
        the blend in front of every stepped row needs q_sample's noise, so its Philox launch covers `noise_q` alone and
        `step(mask_noise=)` fixes that draw;
      * `pred_x0` is always allocated: it is the solver's history, read and rewritten by the step kernel.  Nothing resets it: the first
        stepped row of every table has c_1 = 0 and does not read it, and every trajectory (after `reset`, `encode`, `reinit`,
        `set_schedule`) starts on the first row of its table;
      * the identity rows at the clean end of the table are not stepped (`n_stepped` replays make a trajectory; one more is refused);
      * without guidance (`uc` None or scale 1) the plan holds the B latents and ONE context segment and the step kernel's eps_u is
        NULL, as in `InvertEngine` ('crossattn' models only)."""

    @staticmethod
    def supported(model, x, cond, uc, scale, features_adapter=None):
        """`BaseEngine.supported`, and the unguided call (`uc` None or scale 1.0) under `InvertEngine.supported`'s conditions"""
        if uc is not None and scale != 1.0:
            return BaseEngine.supported(model, x, cond, uc, scale, features_adapter=features_adapter)
        return (_TrajectoryEngine._supports(model, x, [cond]) and "c_crossattn" in cond
                and _TrajectoryEngine._supports_crossattn(model, [cond]))

    @staticmethod
    def key(sampler, x, cond, uc, cfg_scale, features_adapter=None, n_rows=None, mask=None):
        """what an engine built by `DpmEngine(model, sampler, x, cond, uc, cfg_scale, ...)` is good for: `BaseEngine.key`'s entries behind a
        leading "dpmpp" (both share a cache), with the solver's order and `lower_order_final` and the scale bit of the flag word where
        that key holds the sigmas, and no unconditional entries without guidance"""
        guided = uc is not None and cfg_scale != 1.0
        return ("dpmpp", tuple(x.shape), n_ctx(cond), n_ctx(uc) if guided else None, float(cfg_scale) if guided else 1.0,
                sampler.ddim_timesteps.tobytes(), (int(sampler.order), bool(sampler.lower_order_final), bool(sampler.use_scale)),
                str(x.device), tuple(int(c.shape[1]) for c in cond.get("c_concat") or ()),
                None if features_adapter is None else tuple(tuple(f.shape) for f in features_adapter),
                len(sampler.ddim_timesteps) if n_rows is None else int(n_rows), None if mask is None else mask_kind(mask, x.shape))

    def __init__(self, model, sampler, x, cond, uc, cfg_scale, seed=0, features_adapter=None, n_rows=None, mask=None, x0=None):
        S = len(sampler.ddim_timesteps) if n_rows is None else int(n_rows)
        if not 1 <= S <= len(sampler.ddim_timesteps):
            raise ValueError(f"n_rows = {n_rows}: the schedule has {len(sampler.ddim_timesteps)} rows")
        guided = uc is not None and cfg_scale != 1.0
        self.order, self.lower_order_final = int(sampler.order), bool(sampler.lower_order_final)
        self.hybrid = conditioning_key(model) != "crossattn"
        concat = cond.get("c_concat") if self.hybrid else None
        dev, n = self._open(model, x, [cond, uc] if guided else [cond], S, None if concat is None else tuple(int(c.shape[1]) for c in concat),
                            features_adapter)
        self._built = self._schedule_tables(sampler, S)
        self.coef, self.t_table = (t.to(dev) for t in self._built)
        self.it0, self._schedule_set = 0, False
        self.end_iter = dpm_stepped_rows(self._built[0])     # the iteration counter after the last stepped row (`_write_schedule`)
        self.enc_coef = self._built_enc = tuple(c.to(dev) for c in sampler.encode_tables())
        self.enc_state = torch.zeros(8, dtype=torch.int32, device=dev)
        self.model = model
        self._reinit_bufs = None
        self._reinit_src = (None, None)
        self.noise = torch.zeros(n, dtype=torch.float32, device=dev)           # the draws of `encode` / `reinit`; no step reads it
        self.pred_x0 = torch.empty(n, dtype=torch.float32, device=dev)         # the history
        self._open_mask(x, mask, x0)
        self.noise_q = torch.zeros(n, dtype=torch.float32, device=dev) if self.masked else None
        self.reset(x, cond, uc if guided else None, seed, features_adapter=features_adapter, mask=mask, x0=x0)
        plan = self.plan
        flags = _l.MOCA_BASE_MULTISTEP | (_l.MOCA_BASE_SCALE if sampler.use_scale else 0)
        self._wrap_step(self.noise_q, lambda lib, st_, eps_c, eps_u, stream: _l.check(lib.moca_base_ddim_step_f32(
            st_, _l.ptr(plan.x_in), eps_c, eps_u, _l.ptr(self.noise), _l.ptr(self.pred_x0), _l.ptr(self.coef), self.S, float(cfg_scale),
            flags, n, stream), "moca_base_ddim_step_f32"))

    def _schedule_tables(self, sampler, n_rows):
        """`dpmpp_tables` with the order and `lower_order_final` the engine was built with (whatever `sampler` says: `set_schedule`)"""
        return dpmpp_tables(sampler, n_rows, self.order, self.lower_order_final)

    def _write_schedule(self, coef, t_table):
        super()._write_schedule(coef, t_table)
        self.end_iter = self.it0 + dpm_stepped_rows(coef)

    n_stepped = property(lambda self: self.end_iter - self.it0, doc="the steps of a trajectory over the current schedule")

    def step(self, mask_noise=None):
        """one solver step (enqueued, not synchronised); on a masked engine `mask_noise` [B,C,T,H,W] fixes q_sample's draw"""
        if self.n_iter >= self.end_iter:
            raise ValueError(f"the schedule has {self.n_stepped} stepped rows: step {self.n_iter - self.it0} would run past the clean end")
        if mask_noise is not None and not self.masked:
            raise ValueError("mask_noise goes with a masked engine: an unmasked solver step draws nothing")
        with self._step():
            if mask_noise is not None:
                self._fix_noise((self.noise_q, mask_noise))


class InvertEngine(_TrajectoryEngine):
    """One step of deterministic DDIM inversion (`DDIMSampler.encode`) as ONE hipGraph: [timestep rows of step i] + the UNet forward +
    [guidance + update in place, i += 1] -- `BaseEngine`'s two launches around the forward, `moca_base_set_timestep` and
    `moca_base_ddim_step_f32`, on another table.  Step i takes the latents in the plan's input buffer from schedule level
    ddim_alphas_prev[i] to ddim_alphas[i] with the model evaluated at ddim_timesteps[i] (`invert_coef`).  What differs from `BaseEngine`:

      * nothing is drawn: no `moca_fifo_randn_f32` launch.  The step kernel's noise operand is a buffer of zeros that nothing ever
        writes (sigma is 0 in every row, and 0 x an uninitialised NaN would not be 0);
      * the captured kernels read table row S - 1 - iter, so inversion row i is STORED at row S - 1 - i and the iteration counter counts
        up as everywhere.  The rows ascend from the clean end of the schedule, so one engine over the whole schedule serves every
        t_enc <= S: `encode(x0, c, t_enc)` is t_enc steps after a `reset` (no truncated tables as `decode` needs them);
      * without guidance (`uc` None or scale 1: the normal case of inversion) the plan holds the B latents and ONE context segment and
        the step kernel's eps_u is NULL; with guidance 2 B rows with the shared prefix, as `BaseEngine`."""

    @staticmethod
    def supported(model, x, cond, uc=None, scale=1.0):
        """`BaseEngine.supported`'s conditions on the model, the device, the keys and the fps for 'crossattn' models, without its
        `scale != 1.0` clause (the hybrid keys stay on the host-issued path)"""
        branches = [cond] if uc is None or scale == 1.0 else [cond, uc]
        return _TrajectoryEngine._supports(model, x, branches) and "c_crossattn" in cond and _TrajectoryEngine._supports_crossattn(model, branches)

    @staticmethod
    def key(sampler, x, cond, uc=None, cfg_scale=1.0):
        """what an engine built by `InvertEngine(model, sampler, x, cond, uc, cfg_scale)` is good for.  The leading "invert" keeps it
        apart from `BaseEngine.key`'s tuples, which start with a shape, where both share a cache; the engine covers the whole schedule,
        so the number of steps taken is no part of it"""
        guided = uc is not None and cfg_scale != 1.0
        return ("invert", tuple(x.shape), n_ctx(cond), n_ctx(uc) if guided else None, float(cfg_scale) if guided else 1.0,
                sampler.ddim_timesteps.tobytes(), bool(sampler.use_scale), str(x.device))

    def __init__(self, model, sampler, x, cond, uc=None, cfg_scale=1.0, keep_pred_x0=False):
        guided = uc is not None and cfg_scale != 1.0
        dev, n = self._open(model, x, [cond, uc] if guided else [cond], len(sampler.ddim_timesteps))
        self.coef, self.t_table = (t.to(dev) for t in self._schedule_tables(sampler))
        self.zeros = torch.zeros(n, dtype=torch.float32, device=dev)           # the noise operand: sigma = 0 times finite zeros
        self.pred_x0 = torch.empty(n, dtype=torch.float32, device=dev) if keep_pred_x0 else None
        self.reset(x, cond, uc)
        self._wrap_ddim_step(None, self.zeros, cfg_scale, sampler.use_scale)

    @staticmethod
    def _schedule_tables(sampler):
        """host tables over the sampler's whole schedule, inversion row i at table row S - 1 - i: coef [S][8] = {the seven of
        `invert_coef`, unused} and the int64 timesteps"""
        S = len(sampler.ddim_timesteps)
        coef = np.zeros((S, 8), np.float32)
        t_table = np.zeros((S,), np.int64)
        for i in range(S):
            coef[S - 1 - i, :7] = invert_coef(sampler, i)
            t_table[S - 1 - i] = sampler.ddim_timesteps[i]
        return torch.from_numpy(coef), torch.from_numpy(t_table)

    def reset(self, x, cond, uc=None):
        """start the inversion of another clip on the same plan and the same captured graph: latents x0, contexts, fps, step 0"""
        self._refuse_other_shape(x)
        with self._restart(x, cond, uc):
            pass

    def step(self):
        """one inversion step (enqueued, not synchronised)"""
        if self.n_iter >= self.S:
            raise ValueError(f"the schedule has {self.S} levels: step {self.n_iter} would wrap around to the first")
        with self._step():
            pass


def mask_kind(mask, shape):
    """how the DDPM step kernel reads `mask` against latents of `shape`: "c0" (one channel, channel stride 0) or "full"
    (`img_orig * mask`, ddpm3d.py:648, broadcasts: everything else is expanded to the latents' shape)"""
    ms = (1,) * (len(shape) - mask.dim()) + tuple(mask.shape)
    return "c0" if ms[1] == 1 and shape[1] > 1 else "full"


def mask_operand(mask, shape, device):
    """-> (contiguous fp32 mask as the kernel reads it, kernel flag, elements per mask channel)"""
    B, Cc = int(shape[0]), int(shape[1])
    inner = int(np.prod(shape[2:]))
    m = mask.to(device, torch.float32)
    m = m.reshape((1,) * (len(shape) - m.dim()) + tuple(m.shape))
    if mask_kind(mask, shape) == "c0":
        return m.expand(B, 1, *shape[2:]).contiguous(), _l.MOCA_DDPM_MASK_C0, inner
    return m.expand(*shape).contiguous(), 0, inner * Cc


class DdpmEngine(_TrajectoryEngine):
    """One step of `LatentDiffusion.p_sample_loop` (ddpm3d.py:638-648: p_sample at t = i for all samples, then with a mask
    `img = q_sample(x0, ts) * mask + (1 - mask) * img`) as ONE hipGraph: [timestep rows of step k from the state counter
    (`moca_base_set_timestep` over the table arange(timesteps), so step k runs at t = timesteps - 1 - k) + the Philox draws: the step's
    noise and, with a mask, q_sample's, one launch over both] + the UNet forward + [`moca_ddpm_step_f32`, in place, k += 1].  Without
    guidance the plan holds the B latents and one context segment; with it (an extension: the reference's DDPM loop has none) 2 B rows
    with the shared prefix, as `BaseEngine`.  The latents live in the plan's input buffer; `mask` and `x0` are written once per
    trajectory by `reset`.  The step kernel reads its per-sample t from the plan's timestep rows (row stride = frames)."""

    @staticmethod
    def supported(model, x, cond, uc=None):
        """'crossattn' models with `c_crossattn` / `fps` conditioning only (a tensor or a list is `c_crossattn`, as apply_model takes
        them); a guidance branch must have the same keys and fps (the shared prefix adds ONE fps embedding)"""
        if cond is None:
            return False
        branches = [as_cond_dict(c) for c in (cond, uc) if c is not None]
        return _TrajectoryEngine._supports(model, x, branches) and "c_crossattn" in branches[0] and \
            _TrajectoryEngine._supports_crossattn(model, branches)

    @staticmethod
    def key(shape, cond, uc, timesteps, cfg_scale, mask, clip_denoised, parameterization, device):
        """what an engine built by `DdpmEngine(model, x, cond, uc, cfg_scale, timesteps, mask=mask)` is good for: latent shape, context
        lengths (None: no guidance branch), the number of steps, the guidance scale, whether and how a mask is read, the model's
        clip_denoised and parameterization (the kernel's flags) and the device"""
        return (tuple(int(s) for s in shape), n_ctx(cond), None if uc is None else n_ctx(uc), int(timesteps), float(cfg_scale),
                None if mask is None else mask_kind(mask, shape), bool(clip_denoised), str(parameterization), str(device))

    def __init__(self, model, x, cond, uc, cfg_scale, timesteps, mask=None, x0=None, seed=0, keep_x_recon=False):
        self.model = model
        S = int(timesteps)
        if not 1 <= S <= model.num_timesteps:
            raise ValueError(f"timesteps = {timesteps}: the schedule has {model.num_timesteps} rows")
        dev, n = self._open(model, x, [cond] if uc is None else [cond, uc], S)
        self.coef = model._ddpm_dev(dev)["coef"]
        self.t_table = torch.arange(S, dtype=torch.int64, device=dev)           # `for i in reversed(range(0, timesteps))`, :632,639
        self.n = n
        self.n_pad = (n + 3) // 4 * 4                                            # q_sample's draw starts 16-byte aligned
        self.masked = mask is not None
        self.noise = torch.zeros(self.n_pad + n if self.masked else n, dtype=torch.float32, device=dev)
        self.mask = self.x0 = None
        self.mask_inner = 0
        self.flags = model._ddpm_flags(clip=model.clip_denoised)
        if self.masked:
            m, mflag, self.mask_inner = mask_operand(mask, x.shape, dev)
            self.flags |= mflag
            self.mask = torch.empty_like(m)
            self.x0 = torch.empty(n, dtype=torch.float32, device=dev)
        self.x_recon = torch.empty(n, dtype=torch.float32, device=dev) if keep_x_recon else None
        self.reset(x, cond, uc, seed, mask=mask, x0=x0)
        plan, (B, T) = self.plan, (self.shape[0], self.shape[2])
        nq = self.noise[self.n_pad:] if self.masked else None
        self._wrap_step(self.noise, lambda lib, st_, eps_c, eps_u, stream: _l.check(lib.moca_ddpm_step_f32(
            st_, _l.ptr(plan.x_in), _l.ptr(plan.x_in), eps_c, eps_u, _l.ptr(self.noise), _l.ptr(self.x_recon), None, _l.ptr(self.mask),
            _l.ptr(self.x0), _l.ptr(nq), _l.ptr(self.coef), _l.ptr(plan.t_rows), T, B, int(self.coef.shape[0]), n // B, self.mask_inner,
            float(cfg_scale), 1.0, self.flags, stream), "moca_ddpm_step_f32"))

    def reset(self, x, cond, uc=None, seed=0, mask=None, x0=None):
        """start a new trajectory on the same plan: latents x_T, contexts, fps, mask and x0, step 0, a new noise stream"""
        if (uc is not None) != self.guided or (mask is not None) != self.masked:
            raise ValueError("guidance and mask go with an engine built for them")
        self._refuse_other_shape(x)
        with self._restart(x, cond, uc, seed):
            if self.masked:
                m, mflag, inner = mask_operand(mask, self.shape, self.device)
                if m.shape != self.mask.shape or inner != self.mask_inner:
                    raise ValueError(f"mask {tuple(mask.shape)} is read another way than the mask the engine was built with")
                if tuple(x0.shape) != self.shape:
                    raise ValueError(f"x0 {tuple(x0.shape)} does not match the engine's latents {self.shape}")
                self.mask.copy_(m)
                self.x0.copy_(x0.reshape(-1).to(self.device, torch.float32))

    def step(self, noise=None, mask_noise=None):
        """one DDPM step (enqueued, not synchronised); `noise` [B,C,T,H,W] fixes p_sample's draw and, on a masked engine, `mask_noise`
        q_sample's (both or neither: one flag tells the Philox launch that the host filled the buffer)"""
        if self.masked and (noise is None) != (mask_noise is None):
            raise ValueError("a masked engine takes the step's two draws together: noise and mask_noise, or neither")
        with self._step():
            if noise is not None:
                self._fix_noise((self.noise[:self.n], noise), *([(self.noise[self.n_pad:], mask_noise)] if self.masked else []))

    def last_x_recon(self):
        return self._copy(self.x_recon, self.shape)
