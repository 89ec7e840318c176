"""References, case tables and comparison standards of tests/test_step_kernels_cpu.py and tests/test_step_kernels_gpu.py: the device-side
sampling step -- all of csrc/fifo.hip (the MoCA recurrence of one call's windows, fifo_step_kernel / mask_sum_kernel, included), the
base-sampling step (base_set_timestep_kernel / base_step_kernel / state_bump_kernel) of csrc/sampler.hip and the frequency filters
(filter_kernel) of csrc/freeinit.hip.

Every operation is restated in plain torch from the reference's formula (the ddim.py / funcs.py / freeinit_utils.py lines the kernel
comments cite), op by op in the reference's order, with the dtype as a parameter.  These translation units are built with
-ffp-contract=off, so the float32 evaluation IS the expected output, bit for bit (torch.equal); the float64 evaluation is the sanity
line of the float32 one (test_step_kernels_cpu.py prints the worst |fp32 - fp64| / (2^-23 sum of |terms|) per family).  `wrong=` selects
a WRONG restatement (MUTANTS): one per decision a kernel makes; the CPU file shows that every case tells every wrong restatement that
applies to it from the right one, by torch.equal -- the metric of the GPU file.

Mask values come from {0, 0.5, 0.75, 1}: every summation order gives the same fp32 sum, and exactly 0.5 is "not in the mask".

The one measured bound, moca_fifo_randn_f32 (device logf / sqrtf / sincosf): per element against `philox_numpy(..., f32_angle=True)`
-- the float64 evaluation of the SAME fp32-rounded uniforms and fp32-rounded angle 6.2831855f * u2 --

    |got - ref| <= RANDN_BOUND * (2^-23 |ref| + 2^-24 r),        r = sqrt(-2 ln u1)

    measured on an MI355X over all RANDN_CASES (both iterations, both seed halves): worst ratio RANDN_MEASURED = 1.066 (n = 4 * GRID_CAP + 5, iteration 5)
    RANDN_BOUND = 2 * RANDN_MEASURED (another math library may round differently); the project's 2e-4 against the plain float64
    evaluation stays as the outer ceiling.
"""
import math

import numpy as np
import torch

from small_kernels_ref import GRID_CAP, WRAP, edge_items, gen  # noqa: F401  (one definition of the cap and of its edge items)

F32, F64 = torch.float32, torch.float64
HWS = (1, 63, 65, 255, 257, 273)           # below / at / above a wave and a block of 256, and 13 x 21
MASK_VALUES = torch.tensor([0.0, 0.5, 0.75, 1.0])
RANDN_MEASURED = 1.066
RANDN_BOUND = 2 * RANDN_MEASURED
RANDN_CEILING = 2e-4                       # tests/test_loops_gpu.py::test_fifo_randn_kernel_is_philox_box_muller


def sc(v, dtype):
    """a launch argument: the python float rounded to fp32 (what the kernel receives), then widened"""
    return torch.tensor(v, dtype=F32).to(dtype)


def mask_values(g, *shape):
    return MASK_VALUES[torch.randint(0, 4, shape, generator=g)]


def to_ring(lin, head, dim):
    """queue frame j lives in slot (head + j) mod Q (include/moca_hip.h)"""
    return torch.roll(lin, head, dims=dim).contiguous()


def from_ring(ring, head, dim):
    return torch.roll(ring, -head, dims=dim).contiguous()


def flat_scatter(dst, idx, src):
    """dst.flat[idx] = src where idx is inside dst: what an unreduced index does to a flat buffer (its out-of-range part is dropped)"""
    flat, idx, src = dst.reshape(-1), idx.reshape(-1), src.reshape(-1)
    ok = (idx >= 0) & (idx < flat.numel())
    flat[idx[ok]] = src[ok]
    return flat.view(dst.shape)


# ----------------------------------------------------------------------------------------------------------------- guidance
def guidance(e_c, e_u, scale, dtype=F64, wrong=None):
    """ddim.py:304,372: e_t_uncond + scale * (e_t - e_t_uncond); e_u None: no guidance"""
    e_c = e_c.to(dtype)
    if e_u is None:
        return e_c
    e_u = e_u.to(dtype)
    if wrong == "guidance_swapped":
        return e_c + sc(scale, dtype) * (e_u - e_c)
    return e_u + sc(scale, dtype) * (e_c - e_u)


# ----------------------------------------------------------------------------------------------------------------- MoCA step
STEP_ARGS = dict(beta=0.9, one_minus_beta=float(np.float32(1 - 0.9)), gamma=0.5, one_minus_gamma=float(np.float32(1 - 0.5)))
RECURRENCE_WRONGS = ("momentum_at_frame0", "prev_before_momentum", "one_point_five_is_one", "x_prev_after_injection")


def moca_recurrence(x, eps, noise, mom, coef, inject, dtype=F64, wrong=None, beta=0.9, one_minus_beta=0.1, gamma=0.5, one_minus_gamma=0.5):
    """ddim.py:405-430,556-609 over [N][C][F][HW]; coef [N or 1][F][6] = {sqrt(a_t), sqrt(a_prev), sigma_t, sqrt(1 - a_t),
    sqrt(1 - a_prev - sigma_t^2), 2 (1 - t / 1000)}; inject(j, pred_x0) -> pred_x0 is the branch of :565-606.
    Returns (x_prev, pred_x0, momentum); momentum frame 0 is never written (:424 runs for frames i >= 1 only)."""
    x, eps, noise, cf = x.to(dtype), eps.to(dtype), noise.to(dtype), coef.to(dtype)
    mom = mom.to(dtype).clone()
    beta, omb, gamma, omg = (sc(v, dtype) for v in (beta, one_minus_beta, gamma, one_minus_gamma))
    k = lambda j, i: cf[:, j, i].view(-1, 1, 1)
    xps, p0s, prev = [], [], None
    for j in range(x.shape[2]):
        e = eps[:, :, j]
        p0 = (x[:, :, j] - k(j, 3) * e) / k(j, 0)                     # :415
        d = k(j, 4) * e                                               # :418
        if prev is not None or wrong == "momentum_at_frame0":
            g = p0 - (prev if prev is not None else torch.zeros_like(p0))     # :422
            g = g + (1.0 if wrong == "one_point_five_is_one" else 1.5) * d    # :423
            m = beta * mom[:, :, j - 1 if j else 0] + omb * g                  # :424-427
            mom[:, :, j] = m
            if wrong == "prev_before_momentum":
                prev = p0
            p0 = p0 + k(j, 5) * m                                     # :428-430,557
            if wrong != "prev_before_momentum":
                prev = p0                                             # :559
        else:
            prev = p0
        nz = k(j, 2) * noise[:, :, j]                                 # :561
        if wrong == "x_prev_after_injection":
            xps.append(k(j, 1) * inject(j, p0) + d + nz)
        else:
            xps.append(k(j, 1) * p0 + d + nz)                         # :562
        p0 = inject(j, p0)                                            # :565-606
        p0s.append(omg * p0 + gamma * nz)                             # :609
    return torch.stack(xps, 2), torch.stack(p0s, 2), mom


STEP_WRONGS = RECURRENCE_WRONGS + ("mask_ge_half", "mask_batch_stride_f", "minus_one_is_last_frame")


def mask_batch_sums(mask, dtype=F64, wrong=None):
    """ddim.py:585 `mask.sum()` of each mask frame over (batch, pixels): [B][Fm][HW] -> [Fm]"""
    m = mask.to(dtype)
    return m[0].sum(-1) if wrong == "sum_batch0_only" else m.sum((0, 2))


def moca_step(sample, eps, noise, mom, coef, mask, cond, mask_index, enh, dtype=F64, wrong=None, **kw):
    """moca_fifo_ddim_step_f32: one `ddim_step` call over [B][C][F][HW]; mask [B][Fm][HW] (the DAVIS branch :565-590: frame
    mask_index[j] >= 0 is consulted, injected where the frame's sum over the whole batch is not 0 and the video's own pixel > 0.5)"""
    B, C, F, HW = sample.shape
    rw = wrong if wrong in RECURRENCE_WRONGS else None

    def inject(j, p0):
        if mask is None:
            return p0
        mi = int(mask_index[j])
        if mi < 0:
            if wrong != "minus_one_is_last_frame":
                return p0
            mi = mask.shape[1] - 1
        if mask_batch_sums(mask, dtype)[mi] == 0:
            return p0
        if wrong == "mask_batch_stride_f":               # video b's frame at (b F + mi) instead of (b Fm + mi) in the flat buffer
            mk = torch.stack([mask.reshape(-1, HW)[(b * F + mi) % (mask.shape[0] * mask.shape[1])] for b in range(B)])
        else:
            mk = mask[:, mi]
        hit = (mk >= 0.5) if wrong == "mask_ge_half" else (mk > 0.5)
        cnd = torch.zeros_like(p0) if cond is None else cond.to(dtype)
        return torch.where(hit[:, None], cnd * sc(float(enh[j]), dtype), p0)

    return moca_recurrence(sample, eps, noise, mom, coef[None], inject, dtype, rw, **kw)


def _mask_index(F, Fm):
    """-1 entries, repeats, the frame that is zero in batch 0 only (1) and the all-zero frame (3) where there are that many"""
    pat = {1: [1], 2: [1, 0], 8: [1, -1, 2, 2, 4, 0, -1, 3]}[F]
    return torch.tensor([p if p < Fm else -1 for p in pat], dtype=torch.int32)


def _step_cases():
    cases = {}

    def add(name, B, C, F, Fm, HW, mask=True, cond=True, seed=0):
        cases[name] = dict(B=B, C=C, F=F, Fm=Fm, HW=HW, mask=mask, cond=cond, seed=2000 + len(cases))
    add("hw1_b2_c3_f2_fm3", 2, 3, 2, 3, 1)
    add("hw63_b1_c4_f8_fm5", 1, 4, 8, 5, 63)
    add("hw65_b2_c1_f8_fm5", 2, 1, 8, 5, 65)
    add("hw255_b1_c3_f1_fm2", 1, 3, 1, 2, 255)
    add("hw257_b2_c4_f2_fm3", 2, 4, 2, 3, 257)
    add("hw273_b2_c3_f8_fm5", 2, 3, 8, 5, 273)
    add("hw65_b2_c3_f8_fm5_cond_null", 2, 3, 8, 5, 65, cond=False)
    add("hw63_b2_c4_f8_mask_null", 2, 4, 8, 5, 63, mask=False)
    add("wrap_cap_plus_300_b1_c1_f2_fm1", 1, 1, 2, 1, WRAP)
    return cases


STEP_CASES = _step_cases()


def _coef(g, *lead):
    """a coefficient table with every entry different and away from 0 (sqrt(a_t) divides)"""
    return 0.3 + torch.rand(*lead, 6, generator=g)


def step_inputs(c):
    g = gen(c["seed"])
    B, C, F, Fm, HW = c["B"], c["C"], c["F"], c["Fm"], c["HW"]
    t = dict(sample=torch.randn(B, C, F, HW, generator=g), eps=torch.randn(B, C, F, HW, generator=g), noise=torch.randn(B, C, F, HW, generator=g),
             mom=torch.randn(B, C, F, HW, generator=g) * 0.5, coef=_coef(g, F))
    t["cond"] = torch.rand(B, C, HW, generator=g) + 0.25 if c["cond"] else None
    t["mask"] = t["mask_index"] = t["enh"] = None
    if c["mask"]:
        m = mask_values(g, B, Fm, HW)
        m[:, :, 0] = torch.tensor([0.5, 1.0])[:B, None] if B == 2 else 0.5      # exactly 0.5 sits in every frame (with a 1 beside it at B = 2)
        if Fm > 1 and B == 2:
            m[0, 1] = 0.0                                  # zero in batch 0, non-zero in batch 1: the batch-wide sum decides
            m[1, 1, 0] = 1.0
        if Fm > 3:
            m[:, 3] = 0.0                                  # zero everywhere
        t["mask"], t["mask_index"] = m, _mask_index(F, Fm)
        t["enh"] = torch.tensor([1.5, 1.0, 1.5, 1.5, 1.0, 1.5, 1.0, 1.5])[:F].contiguous()
    return t


def step_wrongs(c):
    """prev-before-momentum shows from the third frame on; 1.5 needs a second frame; the mask decisions need a mask; the batch stride
    B = 2 and Fm != F; -1 a -1 entry whose last mask frame is not empty.  (`mask.sum() != 0` itself cannot be told from its absence
    with non-negative masks -- a frame that sums to 0 has no pixel > 0.5: the sums are read back from the workspace instead.)"""
    w = ("momentum_at_frame0", "x_prev_after_injection") if c["mask"] else ("momentum_at_frame0",)
    if c["F"] >= 2:
        w += ("one_point_five_is_one",)
    if c["F"] >= 3:
        w += ("prev_before_momentum",)
    if c["mask"]:
        w += ("mask_ge_half",)
        if c["B"] == 2 and c["Fm"] != c["F"]:
            w += ("mask_batch_stride_f",)
        if c["F"] == 8:
            w += ("minus_one_is_last_frame",)
    return w


def step_eval(c, dtype, wrong=None, t=None):
    t = t or step_inputs(c)
    return moca_step(t["sample"], t["eps"], t["noise"], t["mom"], t["coef"], t["mask"], t["cond"], t["mask_index"], t["enh"], dtype, wrong, **STEP_ARGS)


# ----------------------------------------------------------------------------------------------------------------- segmentation bookkeeping
SAM_WRONGS = ("iou_le_half", "reset_ge_80", "pre_tracks_candidates", "gate_t_lt_300", "iou_over_new_count", "union0_is_zero", "binarise_ge_half")
SAM_SENTINEL = 7.0


def iou_mean_f32(ratios):
    """ddim.py:905-943 as the kernel sums it: sequential fp32 sum of the fp32 ratios, one fp32 division"""
    acc = np.float32(0)
    for r in ratios:
        acc = np.float32(acc + np.float32(r))
    return np.float32(acc / np.float32(len(ratios)))


def sam_select(cands, ts, HW, wrong=None):
    """`_apply_segmentation` (ddim.py:739-903) for precomputed candidates over the frames of ONE `ddim_step` call (`pre_masks = None`
    at its start, :391).  cands[i]: [n_i][HW] fp32 or None (no box detected, :788); ts[i] the frame's timestep (:592 `<= 300`).
    Returns (eff [f][HW] with SAM_SENTINEL rows where nothing is injected, idx [f] = i or -1)."""
    f = len(ts)
    eff = torch.full((f, HW), SAM_SENTINEL)
    idx = np.full((f,), -1, np.int32)
    thr = (lambda m: m >= 0.5) if wrong == "binarise_ge_half" else (lambda m: m > 0.5)
    pre = None
    for i in range(f):
        if (ts[i] >= 300) if wrong == "gate_t_lt_300" else (ts[i] > 300):         # :592
            continue
        cand = cands[i]
        if cand is None or len(cand) == 0:                 # :788-793
            if pre is None:
                continue
            masks = pre
        else:
            masks = cand
            if pre is not None:                            # :804-807, calculate_iou :905-943 over zip(new, previous)
                ratios = []
                for a, b in zip(masks, pre):
                    inter, union = int((thr(a) & thr(b)).sum()), int((thr(a) | thr(b)).sum())
                    ratios.append((0.0 if wrong == "union0_is_zero" else 1.0) if union == 0 else np.float32(inter) / np.float32(union))
                mean = iou_mean_f32(ratios) if wrong != "iou_over_new_count" else np.float32(np.float32(sum(np.float32(r) for r in ratios)) / np.float32(len(masks)))
                if (mean <= 0.5) if wrong == "iou_le_half" else (mean < 0.5):
                    masks = pre
        pre = cand if wrong == "pre_tracks_candidates" and cand is not None and len(cand) else masks
        cur = torch.zeros(HW, dtype=torch.bool)
        big = np.float32(0.8 * HW)                         # `mask.sum() > 0.8 * mask.numel()`: a python float against an fp32 sum (:820)
        for m in masks:
            s = np.float32(m.sum().item())
            if (s >= big) if wrong == "reset_ge_80" else (s > big):
                cur.zero_()                                # modified_pred_x0 = pred_x0 (:821)
                continue
            cur |= thr(m)
        eff[i] = cur.float()
        idx[i] = i
    return eff, idx


def _px(HW, *spans, v=1.0):
    m = torch.zeros(HW)
    for a, b in spans:
        m[a:b] = v
    return m


def _mk(*ms):
    return torch.stack(ms)


def _sam_scripts():
    """windows (= ddim_step calls) of (timestep, candidates) per frame; every window has 4 frames"""
    S = {}
    HW = 260
    z = torch.zeros(HW)
    P = lambda *sp, v=1.0: _px(HW, *sp, v=v)
    S["hw260_iou_exactly_half_taken"] = (HW, [(100, _mk(P((0, 20)))), (100, _mk(P((0, 10), v=0.75))), (100, _mk(P((5, 10)))), (100, None)])
    S["hw260_three_pair_mean_exactly_half_taken"] = (HW, [(100, _mk(P((0, 4)), P((20, 24)), P((40, 44)))),
                                                          (100, _mk(P((3, 4)), P((20, 22)), P((40, 43)))),          # 1/4, 1/2, 3/4
                                                          (100, _mk(P((3, 4)), P((20, 22)), P((40, 43)))), (100, None)])
    S["hw260_sum_exactly_80_percent_no_reset_one_more_resets"] = (HW, [(100, _mk(P((0, 208)))), (100, _mk(P((0, 209)), P((250, 260)))),
                                                                       (100, _mk(P((0, 208)), P((250, 260)))), (100, _mk(torch.maximum(P((0, 208), v=0.5), P((0, 110)))))])
    S["hw260_unequal_pair_counts"] = (HW, [(100, _mk(P((0, 10)))), (100, _mk(P((0, 6)), P((50, 60)), P((70, 80)))),          # 1 pair: 0.6
                                           (100, _mk(P((0, 6)), P((50, 56)))),                                                # 2 pairs: (1 + 0.6) / 2
                                           (100, _mk(P((0, 6)), P((50, 52)), P((70, 80))))])                                  # 2 pairs: (1 + 1/3) / 2
    S["hw260_union_zero_counts_as_one"] = (HW, [(100, _mk(z, P((0, 8)))), (100, _mk(z, P((0, 2)))), (100, _mk(z, z)), (100, _mk(P((0, 1), v=0.5), z))])
    S["hw260_t300_in_t301_out"] = (HW, [(301, _mk(P((0, 9)))), (300, _mk(P((100, 109)))), (301, None), (300, _mk(P((100, 104))))])
    S["hw260_first_frame_without_detection"] = (HW, [(100, None), (100, _mk(P((0, 9)))), (100, None), (100, torch.zeros(0, HW))])
    S["hw260_previous_after_fallback"] = (HW, [(100, _mk(P((0, 20)))), (100, _mk(P((100, 120)))), (100, _mk(P((100, 120)))), (100, _mk(P((0, 12))))])
    for HW in (1, 65):
        P = lambda *sp, v=1.0: _px(HW, *sp, v=v)          # noqa: E731
        h = max(HW // 2, 1)
        S["hw%d_basic" % HW] = (HW, [(100, None), (300, _mk(P((0, h), v=0.75))), (301, _mk(P((0, HW)))), (100, _mk(torch.maximum(P((0, min(h + 1, HW)), v=0.5), P((0, h)))))])
        S["hw%d_full_mask_resets" % HW] = (HW, [(100, _mk(P((0, h)))), (100, _mk(P((0, HW)), P((0, h)))), (100, _mk(P((0, h)), P((0, HW)))), (100, None)])
    S["hw1_half_is_outside"] = (1, [(100, _mk(_px(1, (0, 1), v=0.5))), (100, _mk(_px(1, (0, 1)))), (100, _mk(_px(1, (0, 1), v=0.5))), (100, None)])
    return S


SAM_SCRIPTS = _sam_scripts()
SAM_TELLS = {          # the wrong restatements each scripted window tells
    "hw260_iou_exactly_half_taken": ("iou_le_half",),
    "hw260_three_pair_mean_exactly_half_taken": ("iou_le_half",),
    "hw260_sum_exactly_80_percent_no_reset_one_more_resets": ("reset_ge_80", "binarise_ge_half"),
    "hw260_unequal_pair_counts": ("iou_over_new_count",),
    "hw260_union_zero_counts_as_one": ("union0_is_zero", "binarise_ge_half"),
    "hw260_t300_in_t301_out": ("gate_t_lt_300",),
    "hw260_first_frame_without_detection": (),
    "hw260_previous_after_fallback": ("pre_tracks_candidates",),
    "hw1_basic": ("gate_t_lt_300",), "hw65_basic": ("gate_t_lt_300", "binarise_ge_half"), "hw1_half_is_outside": ("binarise_ge_half",),
    "hw1_full_mask_resets": (), "hw65_full_mask_resets": (),
}


def sam_script(name):
    HW, frames = SAM_SCRIPTS[name]
    return HW, [c for _, c in frames], np.asarray([t for t, _ in frames], np.int64)


def sam_pool(windows, HW):
    """the kernel's arguments for a list of (cands, ts) windows: pool [n][HW], cand_off, ncand, t_rows"""
    pool, off, cnt, ts = [torch.zeros(HW)], [], [], []     # (pool entry 0: never referenced by a frame with candidates)
    for cands, t in windows:
        for c, ti in zip(cands, t):
            n = 0 if c is None else len(c)
            off.append(len(pool) if n else 0)
            cnt.append(n)
            ts.append(int(ti))
            pool.extend(c[k] for k in range(n))
    return torch.stack(pool), torch.tensor(off, dtype=torch.int32), torch.tensor(cnt, dtype=torch.int32), torch.tensor(ts, dtype=torch.int64)


def sam_windows_for(nW, f, HW, seed):
    """nW windows of f frames for the segmentation branch of moca_fifo_step_windows_f32: detections, misses (-1 frames) and t > 300"""
    g = gen(seed)
    out = []
    for w in range(nW):
        cands, ts = [], []
        for i in range(f):
            k = (w + i) % 4
            ts.append(301 if k == 3 else 100)
            cands.append(None if (k == 0 and i < 2) else _mk(mask_values(g, HW)))
        out.append((cands, np.asarray(ts, np.int64)))
    return out


# ----------------------------------------------------------------------------------------------------------------- the windows of an iteration
WIN_WRONGS = RECURRENCE_WRONGS + ("guidance_swapped", "wb_from_off_by_one", "ring_not_mod_q", "wb_head_not_added", "coef_of_window_0",
                                  "mask_slot_not_shifted", "inject_on_zero_sum", "mask_ge_half", "seg_uses_enh", "seg_ignores_idx")


def gather_windows(queue, head, starts, f, reps, dtype=F64, wrong=None):
    """funcs.py:315 `latents[:, :, start:end].clone()` on the ring [C][Q][HW], repeated for the unconditional branch (ddim.py:366-369):
    x [reps][nW][C][f][HW]; funcs.py:88: anchor [C][HW] = queue frame 0"""
    C, Q, HW = queue.shape
    q = queue.to(dtype)
    xs = []
    for s0 in starts:
        fr = torch.arange(f) + int(s0) + (0 if wrong == "head_not_added" else head)
        if wrong == "ring_not_mod_q":                      # frame index past Q in the flat [C][Q][HW] buffer
            flat = torch.cat([q.reshape(-1), torch.full((f * HW,), float("nan"), dtype=dtype)])
            idx = ((torch.arange(C)[:, None, None] * Q + fr[None, :, None]) * HW + torch.arange(HW)[None, None]).clamp(max=flat.numel() - 1)
            xs.append(flat[idx])
        else:
            xs.append(q[:, fr % Q])
    x = torch.stack(xs)
    anchor = q[:, (head + Q - 1) % Q] if wrong == "anchor_from_tail" else q[:, head]
    if wrong == "reps_share_one_copy":
        return torch.cat([x[None], torch.zeros_like(x[None]).expand(reps - 1, *x.shape)]), anchor
    return x[None].expand(reps, *x.shape).contiguous(), anchor


def step_windows(x, e_c, e_u, noise, mom, coef, queue, head, starts, wb_from, cfg_scale, mask=None, mask_sums=None, mask_frame=None, enh=None,
                 cond=None, sam_eff=None, sam_idx=None, dtype=F64, wrong=None, **kw):
    """moca_fifo_step_windows_f32: guidance (:372) + `ddim_step` of every window [nW][C][f][HW] + the write-back of funcs.py:351-354
    (`latents[:, :, start + wb_from:end] = x_prev[:, :, wb_from:]`) into the ring [C][Q][HW].  mask [Q][HW] / mask_sums [Q] are rings
    too: queue frame mask_frame[w][j] >= 0 is consulted (:565-590); else the segmentation masks sam_eff [nW][f][HW] where
    sam_idx[w][j] >= 0, factor 2 (:592-606 -> :847,897-901).  Returns (x_prev, pred_x0, momentum, queue)."""
    nW, C, f, HW = x.shape
    rw = wrong if wrong in RECURRENCE_WRONGS else None
    eps = guidance(e_c, e_u, cfg_scale, dtype, wrong)
    cf = coef[:1].expand(nW, -1, -1) if wrong == "coef_of_window_0" else coef

    def inject(j, p0):
        cnd = torch.zeros((C, HW), dtype=dtype) if cond is None else cond.to(dtype)
        out = p0.clone()
        for w in range(nW):
            mf = int(mask_frame[w, j]) if mask is not None else -1
            if mf >= 0:
                ms = (mf if wrong == "mask_slot_not_shifted" else head + mf) % mask.shape[0]
                if mask_sums[ms] != 0 or wrong == "inject_on_zero_sum":
                    hit = (mask[ms] >= 0.5) if wrong == "mask_ge_half" else (mask[ms] > 0.5)
                    out[w] = torch.where(hit[None], cnd * sc(float(enh[w, j]), dtype), p0[w])
            elif sam_eff is not None and (int(sam_idx[w, j]) >= 0 or wrong == "seg_ignores_idx"):
                fac = sc(float(enh[w, j]), dtype) if wrong == "seg_uses_enh" else 2.0
                out[w] = torch.where((sam_eff[w, j] > 0.5)[None], cnd * fac, p0[w])
        return out

    xp, p0, mom = moca_recurrence(x, eps, noise, mom, cf, inject, dtype, rw, **kw)
    if queue is None:
        return xp, p0, mom, None
    q = queue.to(dtype).clone()
    Q = q.shape[1]
    for w, s0 in enumerate(starts):
        for j in range(f):
            if (j > wb_from) if wrong == "wb_from_off_by_one" else (j >= wb_from):
                fr = int(s0) + j + (0 if wrong == "wb_head_not_added" else head)
                if wrong == "ring_not_mod_q":
                    idx = (torch.arange(C)[:, None] * Q + fr) * HW + torch.arange(HW)[None]
                    q = flat_scatter(q, idx, xp[w, :, j])
                else:
                    q[:, fr % Q] = xp[w, :, j]
    return xp, p0, mom, q


def _win_cases():
    cases = {}

    def add(name, Q, f, head, starts, wb, HW, C, branch=None, eps_u=True, x_prev=True, pred_x0=True, queue=True):
        cases[name] = dict(Q=Q, f=f, head=head, starts=starts, wb_from=wb, HW=HW, C=C, branch=branch, eps_u=eps_u, x_prev=x_prev,
                           pred_x0=pred_x0, queue=queue, seed=3000 + len(cases))
    add("q_eq_f_head0_wb0_hw63_c3_mask", 4, 4, 0, [0], 0, 63, 3, "mask")
    add("q_eq_f_head_last_straddles_wb_half_hw1_c4", 4, 4, 3, [0], 2, 1, 4)
    add("q_f_plus_1_head2_overlapping_wb_f_hw65_c1_seg", 5, 4, 2, [0, 1], 4, 65, 1, "seg")
    add("q_f_plus_1_head_last_wb_half_hw255_c3_mask_eps_u_null", 5, 4, 4, [1], 2, 255, 3, "mask", eps_u=False)
    add("q20_head13_straddles_wb_half_hw257_c4_mask_zero_sum_slot", 20, 8, 13, [12, 8, 4, 0], 4, 257, 4, "mask")
    add("q20_head0_disjoint_wb0_hw273_c3_seg", 20, 8, 0, [0, 8], 0, 273, 3, "seg")
    add("q20_head_last_wb_half_hw65_c3_x_prev_null", 20, 8, 19, [12, 8, 4, 0], 4, 65, 3, x_prev=False)
    add("q20_head5_wb_half_hw63_c4_pred_x0_null", 20, 8, 5, [12, 8, 4, 0], 4, 63, 4, pred_x0=False)
    add("queue_null_hw255_c1_seg", 20, 8, 7, [3, 0], 4, 255, 1, "seg", queue=False)
    add("wrap_cap_plus_300_q_eq_f_head1_wb0_mask", 2, 2, 1, [0], 0, WRAP, 1, "mask")
    return cases


WIN_CASES = _win_cases()


def win_inputs(c):
    g = gen(c["seed"])
    Q, f, HW, C, head, starts = c["Q"], c["f"], c["HW"], c["C"], c["head"], c["starts"]
    nW = len(starts)
    t = dict(queue_lin=torch.randn(C, Q, HW, generator=g), e_c=torch.randn(nW, C, f, HW, generator=g), noise=torch.randn(nW, C, f, HW, generator=g),
             mom=torch.randn(nW, C, f, HW, generator=g) * 0.5, coef=_coef(g, nW, f), cond=torch.rand(C, HW, generator=g) + 0.25)
    t["e_u"] = torch.randn(nW, C, f, HW, generator=g) if c["eps_u"] else None
    t["queue"] = to_ring(t["queue_lin"], head, 1)
    t["x"] = gather_windows(t["queue"], head, starts, f, 1, F32)[0][0]
    t["enh"] = torch.tensor([1.5, 1.0])[torch.randint(0, 2, (nW, f), generator=g)]
    t["enh"][:, :2] = torch.tensor([1.5, 1.0])
    t["mask"] = t["mask_sums"] = t["mask_frame"] = t["sam_eff"] = t["sam_idx"] = None
    if c["branch"] == "mask":
        lin = mask_values(g, Q, HW)
        lin[:, 0] = 0.5
        if HW > 1:
            lin[:, 1] = 1.0
        mf = torch.stack([torch.tensor([s0 + j if (j + w) % 3 else -1 for j in range(f)]) for w, s0 in enumerate(starts)]).to(torch.int32)
        mf[0, 0], mf[0, 1] = starts[0], starts[0] + 1
        t["mask"], t["mask_frame"] = to_ring(lin, head, 0), mf
        sums = t["mask"].sum(1)
        sums[(head + starts[0] + 1) % Q] = 0.0             # a consulted ring slot whose CARRIED sum is 0 although its pixels are not
        t["mask_sums"] = sums
    elif c["branch"] == "seg":
        wins = sam_windows_for(nW, f, HW, c["seed"] + 500)
        t["sam_pool"] = sam_pool(wins, HW)
        sel = [sam_select(cd, ts, HW) for cd, ts in wins]
        t["sam_eff"] = torch.stack([e for e, _ in sel])
        t["sam_idx"] = torch.from_numpy(np.stack([i for _, i in sel]))
    return t


def win_wrongs(c):
    nW, f, Q, head = len(c["starts"]), c["f"], c["Q"], c["head"]
    w = ("momentum_at_frame0", "one_point_five_is_one") + (("prev_before_momentum",) if f >= 3 else ())
    if c["branch"] and c["pred_x0"] and c["x_prev"]:
        w += ("x_prev_after_injection",)
    if c["eps_u"]:
        w += ("guidance_swapped",)
    if nW > 1:
        w += ("coef_of_window_0",)
    if c["queue"]:
        written = [head + s0 + j for s0 in c["starts"] for j in range(c["wb_from"], f)]
        if c["wb_from"] < f:
            w += ("wb_from_off_by_one",)
        if any(fr >= Q for fr in written):
            w += ("ring_not_mod_q",)
        if written and head:
            w += ("wb_head_not_added",)
    if c["branch"] == "mask" and c["pred_x0"]:
        w += ("inject_on_zero_sum", "mask_ge_half") + (("mask_slot_not_shifted",) if head else ())
    if c["branch"] == "seg" and c["pred_x0"]:
        w += ("seg_uses_enh", "seg_ignores_idx")
    return w


WIN_ARGS = dict(cfg_scale=12.0, **STEP_ARGS)


def win_eval(c, dtype, wrong=None, t=None):
    t = t or win_inputs(c)
    xp, p0, mom, q = step_windows(t["x"], t["e_c"], t["e_u"], t["noise"], t["mom"], t["coef"], t["queue"] if c["queue"] else None, c["head"], c["starts"],
                                  c["wb_from"], mask=t["mask"], mask_sums=t["mask_sums"], mask_frame=t["mask_frame"], enh=t["enh"], cond=t["cond"],
                                  sam_eff=t["sam_eff"], sam_idx=t["sam_idx"], dtype=dtype, wrong=wrong, **WIN_ARGS)
    return dict(x_prev=xp if c["x_prev"] else None, pred_x0=p0 if c["pred_x0"] else None, mom=mom, queue=q)


GATHER_WRONGS = ("ring_not_mod_q", "head_not_added", "anchor_from_tail", "reps_share_one_copy")


def _gather_cases():
    cases = {}

    def add(name, Q, f, head, starts, reps, HW, C, x=True, anchor=True):
        cases[name] = dict(Q=Q, f=f, head=head, starts=starts, reps=reps, HW=HW, C=C, x=x, anchor=anchor, seed=3500 + len(cases))
    add("q_eq_f_head0_reps1_hw63_c3", 4, 4, 0, [0], 1, 63, 3)
    add("q_eq_f_head_last_reps2_hw1_c4", 4, 4, 3, [0], 2, 1, 4)
    add("q_f_plus_1_head2_overlapping_reps2_hw65_c1", 5, 4, 2, [0, 1], 2, 65, 1)
    add("q_f_plus_1_head_last_reps1_hw255_c3_no_anchor", 5, 4, 4, [1, 0], 1, 255, 3, anchor=False)
    add("q20_head13_straddles_overlapping_reps2_hw257_c4", 20, 8, 13, [12, 8, 4, 0], 2, 257, 4)
    add("q20_head0_reps1_hw273_c3", 20, 8, 0, [12, 8, 4, 0], 1, 273, 3)
    add("q20_head_last_anchor_alone_hw65_c3", 20, 8, 19, [], 1, 65, 3, x=False)
    add("wrap_cap_plus_300_q2_f1_head1_reps2", 2, 1, 1, [1], 2, WRAP, 1)
    return cases


GATHER_CASES = _gather_cases()


def gather_wrongs(c):
    w = ()
    if c["x"]:
        if any(c["head"] + s0 + c["f"] > c["Q"] for s0 in c["starts"]):
            w += ("ring_not_mod_q",)
        if c["head"]:
            w += ("head_not_added",)
        if c["reps"] > 1:
            w += ("reps_share_one_copy",)
    return w + (("anchor_from_tail",) if c["anchor"] and c["Q"] > 1 else ())


def gather_eval(c, dtype=F32, wrong=None):
    q = torch.randn(c["C"], c["Q"], c["HW"], generator=gen(c["seed"]))
    x, a = gather_windows(q, c["head"], c["starts"] or [0], c["f"], c["reps"], dtype, wrong)
    return q, (x if c["x"] else None), (a if c["anchor"] else None)


# ----------------------------------------------------------------------------------------------------------------- advance
ADV_WRONGS = ("emit_after_overwrite", "slot_iter_plus_1", "mask_tail_not_kept", "mask_sums_not_carried", "emit_without_head")


def advance(state, queue, newframe, emitted, n_slots, emit_frame, mask, mask_sums, wrong=None):
    """funcs.py:357-371 minus the decode, on the rings: emitted[iter mod n_slots] = queue frame emit_frame; the slot of the dequeued
    frame 0 receives `newframe` (funcs.py:97) and becomes the tail; the mask ring keeps its last frame (funcs.py:113-116) and its sum;
    head + 1 mod Q, iter + 1, ext_noise = 0.  state = (head, iter, ext_noise); returns the same tuple of new values."""
    head, it, _ = state
    Q = queue.shape[1]
    queue = queue.clone()
    ef, tail = ((0 if wrong == "emit_without_head" else head) + emit_frame) % Q, (head + Q - 1) % Q
    if emitted is not None:
        emitted = emitted.clone()
        slot = (it + 1 if wrong == "slot_iter_plus_1" else it) % n_slots
        if wrong == "emit_after_overwrite":
            queue[:, head] = newframe
        emitted[slot] = queue[:, ef]
    queue[:, head] = newframe
    if mask is not None:
        mask, mask_sums = mask.clone(), mask_sums.clone()
        if wrong != "mask_tail_not_kept":
            mask[head] = mask[tail]
        if wrong != "mask_sums_not_carried":
            mask_sums[head] = mask_sums[tail]
    return ((head + 1) % Q, it + 1, 0), queue, emitted, mask, mask_sums


def _adv_cases():
    cases = {}

    def add(name, Q, ef, head, it, HW, C, emitted=True, mask=True, n_slots=3):
        cases[name] = dict(Q=Q, emit_frame=ef, head=head, iter=it, HW=HW, C=C, emitted=emitted, mask=mask, n_slots=n_slots, seed=4000 + len(cases))
    add("emit0_head0_iter0_hw63_c3", 20, 0, 0, 0, 63, 3)
    add("emit0_head_last_iter_last_slot_hw1_c4", 20, 0, 19, 2, 1, 4)
    add("emit_half_head0_iter_n_slots_hw65_c1", 20, 4, 0, 3, 65, 1)
    add("emit_half_head_last_iter_2n_plus_1_hw255_c3", 20, 4, 19, 7, 255, 3)
    add("emit_last_head0_iter_last_slot_hw257_c4", 20, 19, 0, 2, 257, 4)
    add("emit_last_head_last_iter_n_slots_hw273_c3", 20, 19, 19, 3, 273, 3)
    add("emitted_null_hw65_c3", 20, 4, 13, 1, 65, 3, emitted=False)
    add("mask_null_hw63_c4", 20, 4, 13, 7, 63, 4, mask=False)
    add("q1_hw65_c3", 1, 0, 0, 4, 65, 3)
    add("wrap_cap_plus_300_q2_emit0_head1", 2, 0, 1, 5, WRAP, 1)
    return cases


ADV_CASES = _adv_cases()


def adv_wrongs(c):
    w = ()
    if c["emitted"]:
        w += ("slot_iter_plus_1",)
        if c["emit_frame"] == 0:
            w += ("emit_after_overwrite",)
        if c["head"] and c["Q"] > 1:
            w += ("emit_without_head",)
    if c["mask"] and c["Q"] > 1:
        w += ("mask_tail_not_kept", "mask_sums_not_carried")
    return w


def adv_inputs(c):
    g = gen(c["seed"])
    Q, HW, C = c["Q"], c["HW"], c["C"]
    mask = mask_values(g, Q, HW) if c["mask"] else None
    if mask is not None:
        mask[:, 0] = torch.arange(Q) % 4 * 0.25 + 0.25 * (torch.arange(Q) % 4 == 1)      # neighbouring slots differ in pixel 0 and in their sums
    return dict(queue=torch.randn(C, Q, HW, generator=g), newframe=torch.randn(C, HW, generator=g),
                newframe2=torch.randn(C, HW, generator=g), emitted=torch.randn(c["n_slots"], C, HW, generator=g) if c["emitted"] else None,
                mask=mask, mask_sums=(mask.sum(1) + torch.arange(Q)) if c["mask"] else None)


def adv_eval(c, wrong=None, t=None):
    """two calls in a row (the second sees the bumped state and emits frame emit_frame of the shifted queue)"""
    t = t or adv_inputs(c)
    st, q, e, m, ms = advance((c["head"], c["iter"], 1), t["queue"], t["newframe"], t["emitted"], c["n_slots"], c["emit_frame"], t["mask"], t["mask_sums"], wrong)
    first = (st, q, e, m, ms)
    return first, advance(st, q, t["newframe2"], e, c["n_slots"], c["emit_frame"], m, ms, wrong)


# ----------------------------------------------------------------------------------------------------------------- queue preparation
PREP_WRONGS = ("coef_by_source_frame", "frame_idx_ignored", "noise_of_source_frame")


def prepare_queue(z, noise, ca, cb, fidx, dtype=F64, wrong=None):
    """funcs.py:53-79: queue frame j = alpha_j ** 0.5 * z[:, :, frame_idx_j] + (1 - alpha_j) ** 0.5 * noise_j; z [BC][Tz][HW], noise [BC][Q][HW]"""
    z, noise, ca, cb = z.to(dtype), noise.to(dtype), ca.to(dtype), cb.to(dtype)
    Q, Tz = noise.shape[1], z.shape[1]
    fi = fidx.long()
    src = torch.arange(Q).clamp(max=Tz - 1) if wrong == "frame_idx_ignored" else fi
    a = (ca[fi % Q] if wrong == "coef_by_source_frame" else ca)[None, :, None] * z[:, src]
    b = cb[None, :, None] * (noise[:, fi % Q] if wrong == "noise_of_source_frame" else noise)
    return a + b


def _prep_cases():
    cases = {}

    def add(name, BC, Tz, Q, HW):
        cases[name] = dict(BC=BC, Tz=Tz, Q=Q, HW=HW, seed=4500 + len(cases))
    add("bc1_tz1_q5_hw1", 1, 1, 5, 1)
    add("bc8_tz3_q5_hw63", 8, 3, 5, 63)
    add("bc8_tz16_q20_hw65", 8, 16, 20, 65)
    add("bc1_tz3_q20_hw255", 1, 3, 20, 255)
    add("bc8_tz1_q4_hw257", 8, 1, 4, 257)
    add("bc1_tz16_q20_hw273", 1, 16, 20, 273)
    add("wrap_cap_plus_300_bc1_tz1_q2", 1, 1, 2, WRAP)
    return cases


PREP_CASES = _prep_cases()


def prep_inputs(c):
    g = gen(c["seed"])
    BC, Tz, Q, HW = c["BC"], c["Tz"], c["Q"], c["HW"]
    fidx = torch.tensor([max(0, j - (Q - Tz)) for j in range(Q)], dtype=torch.int32)      # funcs.py:63: repeats of frame 0, then every frame
    if Tz > 1:
        fidx[0] = Tz - 1                                                                  # the last source frame, first
        fidx[Q - 1] = Tz - 2
    return dict(z=torch.randn(BC, Tz, HW, generator=g), noise=torch.randn(BC, Q, HW, generator=g), ca=0.3 + torch.rand(Q, generator=g),
                cb=0.3 + torch.rand(Q, generator=g), fidx=fidx)


def prep_wrongs(c):
    return ("coef_by_source_frame", "noise_of_source_frame") + (("frame_idx_ignored",) if c["Tz"] > 1 else ())


def prep_eval(c, dtype, wrong=None, t=None):
    t = t or prep_inputs(c)
    return prepare_queue(t["z"], t["noise"], t["ca"], t["cb"], t["fidx"], dtype, wrong)


# ----------------------------------------------------------------------------------------------------------------- base sampling
BASE_WRONGS = ("row_iter_mod_s", "guidance_swapped", "scale_ignored", "scale_prev_ignored")


def schedule_row(it, S, wrong=None):
    """ddim.py:238: step i of the loop uses schedule index S - 1 - i, i = iter mod S"""
    return it % S if wrong == "row_iter_mod_s" else S - 1 - it % S


def base_step(x, e_c, e_u, noise, coef, it, S, cfg_scale, use_scale, dtype=F64, wrong=None):
    """guidance (ddim.py:304) + the tail of p_sample_ddim (:328-357); coef [S][8] = {sqrt(a_t), sqrt(a_prev), sigma_t, sqrt(1 - a_t),
    sqrt(1 - a_prev - sigma_t^2), scale_t, scale_prev, -}.  Returns (x_prev, pred_x0)."""
    cf = coef[schedule_row(it, S, wrong)].to(dtype)
    e = guidance(e_c, e_u, cfg_scale, dtype, wrong)
    x, noise = x.to(dtype), noise.to(dtype)
    p0 = (x - cf[3] * e) / cf[0]                           # :339
    d = cf[4] * e                                          # :343
    nz = cf[2] * noise                                     # :345
    if use_scale and wrong != "scale_ignored":
        p0 = p0 / cf[5]                                    # :353
        xp = (cf[1] if wrong == "scale_prev_ignored" else cf[1] * cf[6]) * p0 + d + nz     # :354
    else:
        xp = cf[1] * p0 + d + nz                           # :356
    return xp, p0


def _base_cases():
    cases = {}

    def add(name, S, it, use_scale, n, eps_u=True, pred_x0=True):
        cases[name] = dict(S=S, iter=it, use_scale=use_scale, n=n, eps_u=eps_u, pred_x0=pred_x0, seed=5000 + len(cases))
    add("s1_iter0_scale1_n1", 1, 0, 1, 1)
    add("s1_iter5_scale0_n255", 1, 5, 0, 255)
    add("s6_iter0_scale1_n257", 6, 0, 1, 257)
    add("s6_iter_last_scale0_n255", 6, 5, 0, 255)
    add("s6_iter_s_scale1_n257_eps_u_null", 6, 6, 1, 257, eps_u=False)
    add("s6_iter_2s_plus_3_scale0_n1_pred_x0_null", 6, 15, 0, 1, pred_x0=False)
    add("s6_iter_2s_plus_3_scale1_n255", 6, 15, 1, 255)
    add("wrap_cap_plus_300_s6_iter_s_scale1", 6, 6, 1, WRAP)
    return cases


BASE_CASES = _base_cases()
BASE_CFG = 7.5


def base_inputs(c):
    g = gen(c["seed"])
    n = c["n"]
    return dict(x=torch.randn(n, generator=g), e_c=torch.randn(n, generator=g), e_u=torch.randn(n, generator=g) if c["eps_u"] else None,
                noise=torch.randn(n, generator=g), coef=0.3 + torch.rand(c["S"], 8, generator=g))


def base_wrongs(c):
    w = ("row_iter_mod_s",) if c["S"] > 1 and schedule_row(c["iter"], c["S"]) != c["iter"] % c["S"] else ()
    w += ("guidance_swapped",) if c["eps_u"] else ()
    return w + (("scale_ignored", "scale_prev_ignored") if c["use_scale"] else ())


def base_eval(c, dtype, wrong=None, t=None):
    t = t or base_inputs(c)
    return base_step(t["x"], t["e_c"], t["e_u"], t["noise"], t["coef"], c["iter"], c["S"], BASE_CFG, c["use_scale"], dtype, wrong)


TIMESTEP_ROW_CASES = {"s1_iter0_rows1": dict(S=1, iter=0, n=1), "s6_iter0_rows257": dict(S=6, iter=0, n=257), "s6_iter_last_rows1": dict(S=6, iter=5, n=1),
                      "s6_iter_s_rows257": dict(S=6, iter=6, n=257), "s6_iter_2s_plus_3_rows257": dict(S=6, iter=15, n=257),
                      "wrap_cap_plus_300_s6_iter_2s_plus_3": dict(S=6, iter=15, n=WRAP)}


def timestep_table(S):
    return (torch.arange(S, dtype=torch.int64) * 167 + 1) * (1 << 33) + 5          # (every row different in both 32-bit halves)


# ----------------------------------------------------------------------------------------------------------------- mask frame sums
def mask_frame_sums(mask, dtype=F64, wrong=None):
    """the `mask.sum()` of ddim.py:585 per frame of a [frames][HW] mask"""
    m = mask.to(dtype)
    HW = m.shape[1]
    return (m[:, :HW - 1] if wrong == "last_pixel_dropped" else m).sum(-1)


def sums_inputs(HW, seed):
    m = mask_values(gen(seed), 5, HW)
    m[1] = 0.0                                             # all zero
    m[2] = 0.0
    m[2, HW - 1] = 0.75                                    # a single pixel: the last one
    m[:, HW - 1] = torch.where(m[:, HW - 1] == 0, torch.tensor(0.5), m[:, HW - 1])
    m[1] = 0.0
    return m


# ----------------------------------------------------------------------------------------------------------------- Philox + Box-Muller
def philox_numpy(seed, it, n, f32_angle=False, with_r=False):
    """Philox4x32-10, counter (i, i >> 32, iteration, 0x4d6f4341), key = seed words; Box-Muller like csrc/fifo.hip.  The uniforms are
    the kernel's fp32 values; log, sqrt, cos, sin in float64.  f32_angle: the angle 6.2831855f * u2 is rounded to fp32 as well (the
    kernel's sincosf argument), so that only the device logf / sqrtf / sincosf error remains.  with_r: also r = sqrt(-2 ln u1) per element."""
    n4 = (n + 3) // 4
    c = np.zeros((n4, 4), np.uint64)
    c[:, 0] = np.arange(n4) & 0xffffffff
    c[:, 1] = np.arange(n4) >> 32
    c[:, 2] = it
    c[:, 3] = 0x4d6f4341
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    M = np.uint64(0xffffffff)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[:, 0]
        p1 = np.uint64(0xCD9E8D57) * c[:, 2]
        n0 = ((p1 >> np.uint64(32)) ^ c[:, 1] ^ k0) & M
        n2 = ((p0 >> np.uint64(32)) ^ c[:, 3] ^ k1) & M
        c = np.stack([n0, p1 & M, n2, p0 & M], 1)
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    u = (c.astype(np.float32) + np.float32(0.5)) * np.float32(2.3283064365386963e-10)
    out = np.zeros((n4, 4), np.float64)
    rs = np.zeros((n4, 4), np.float64)
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(u[:, 2 * h].astype(np.float64)))
        if f32_angle:
            th = (np.float32(6.283185307179586) * u[:, 2 * h + 1]).astype(np.float64)
        else:
            th = 6.283185307179586 * u[:, 2 * h + 1].astype(np.float64)
        out[:, 2 * h], out[:, 2 * h + 1] = r * np.cos(th), r * np.sin(th)
        rs[:, 2 * h] = rs[:, 2 * h + 1] = r
    if with_r:
        return out.reshape(-1)[:n], rs.reshape(-1)[:n]
    return out.reshape(-1)[:n]


RANDN_SEED = 0x1234567_89abcdef
RANDN_CASES = {"n%d" % n: n for n in (1, 2, 3, 4, 5, 1023)}
RANDN_CASES["wrap_4_caps_plus_5"] = 4 * GRID_CAP + 5


def randn_ratio(got, ref, r):
    """|err| in units of the bound; where u1 rounds to 1 (r = 0: both outputs are exactly 0) any difference is infinitely far"""
    err, den = np.abs(got.astype(np.float64) - ref), 2.0 ** -23 * np.abs(ref) + 2.0 ** -24 * r
    return np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0))


# ----------------------------------------------------------------------------------------------------------------- frequency filters
FILTER_TYPES = {"gaussian": 0, "butterworth": 1, "ideal": 2, "box": 3}
FILTER_WRONGS = ("box_threshold_half_up", "box_threshold_half_down", "ds_dt_exchanged", "zero_cutoff_not_zeros")


def _round_half_up(v):
    return int(math.floor(v + 0.5))


def _round_half_down(v):
    return int(math.ceil(v - 0.5))


def freq_filter(T, H, W, kind, n, d_s, d_t, wrong=None):
    """freeinit_utils.py:73-156 in Python floats, loop by loop as the reference computes them, then rounded to fp32 (the reference
    assigns into a torch.zeros fp32 volume).  Volumes above 2^16 bins are evaluated with the same expressions on float64 numpy grids."""
    out = np.zeros((T, H, W), np.float64)
    if (d_s == 0 or d_t == 0) and wrong != "zero_cutoff_not_zeros":                       # :84,106,127,148
        return torch.from_numpy(out.astype(np.float32))
    if wrong == "zero_cutoff_not_zeros" and (d_s == 0 or d_t == 0):
        d_s, d_t = d_s or 0.25, d_t or 0.25
    if wrong == "ds_dt_exchanged":
        d_s, d_t = d_t, d_s
    if kind == "box":                                                                      # :151-155
        rnd = {"box_threshold_half_up": _round_half_up, "box_threshold_half_down": _round_half_down}.get(wrong, round)
        th, tt = rnd(int(H // 2) * d_s), rnd(T // 2 * d_t)
        cf, cr, cc = T // 2, H // 2, W // 2
        out[cf - tt:cf + tt, cr - th:cr + th, cc - th:cc + th] = 1.0
        return torch.from_numpy(out.astype(np.float32))
    if T * H * W > 1 << 16:
        t, h, w = (np.arange(k, dtype=np.float64) for k in (T, H, W))
        d2 = (((d_s / d_t) * (2 * t / T - 1)) ** 2)[:, None, None] + ((2 * h / H - 1) ** 2)[None, :, None] + ((2 * w / W - 1) ** 2)[None, None]
        if kind == "gaussian":
            out = np.exp(-1 / (2 * d_s ** 2) * d2)
        elif kind == "butterworth":
            out = 1 / (1 + (d2 / d_s ** 2) ** n)
        else:
            out = (d2 <= d_s * 2).astype(np.float64)
        return torch.from_numpy(out.astype(np.float32))
    for t in range(T):
        for h in range(H):
            for w in range(W):
                d_square = (((d_s / d_t) * (2 * t / T - 1)) ** 2 + (2 * h / H - 1) ** 2 + (2 * w / W - 1) ** 2)
                if kind == "gaussian":
                    out[t, h, w] = math.exp(-1 / (2 * d_s ** 2) * d_square)               # :90
                elif kind == "butterworth":
                    out[t, h, w] = 1 / (1 + (d_square / d_s ** 2) ** n)                   # :112
                else:
                    out[t, h, w] = 1 if d_square <= d_s * 2 else 0                        # :133
    return torch.from_numpy(out.astype(np.float32))


def ideal_margin(T, H, W, d_s, d_t):
    """min |d^2 - 2 d_s| over the bins where the two are not equal in double arithmetic"""
    t, h, w = (np.arange(k, dtype=np.float64) for k in (T, H, W))
    d2 = (((d_s / d_t) * (2 * t / T - 1)) ** 2)[:, None, None] + ((2 * h / H - 1) ** 2)[None, :, None] + ((2 * w / W - 1) ** 2)[None, None]
    gap = np.abs(d2 - d_s * 2)
    return gap[gap != 0].min() if (gap != 0).any() else np.inf


def _filter_cases():
    cases = {}
    shapes = ((1, 1, 1), (3, 5, 7), (16, 10, 12), (4, 20, 6))
    for kind in FILTER_TYPES:
        for T, H, W in shapes:
            cases["%s_t%d_h%d_w%d" % (kind, T, H, W)] = dict(kind=kind, shape=(T, H, W), n=4, d_s=0.25, d_t=0.25)
        cases["%s_t16_h10_w12_ds_ne_dt" % kind] = dict(kind=kind, shape=(16, 10, 12), n=2, d_s=0.5, d_t=0.25)
        cases["%s_t4_h20_w6_ds_zero" % kind] = dict(kind=kind, shape=(4, 20, 6), n=4, d_s=0.0, d_t=0.25)
        cases["%s_t3_h5_w7_dt_zero" % kind] = dict(kind=kind, shape=(3, 5, 7), n=4, d_s=0.25, d_t=0.0)
    cases["box_t4_h10_w12_threshold_2_5"] = dict(kind="box", shape=(4, 10, 12), n=4, d_s=0.5, d_t=0.25)      # H/2 d_s = 2.5 -> 2; T/2 d_t = 0.5 -> 0
    cases["box_t8_h20_w12_threshold_2_5"] = dict(kind="box", shape=(8, 20, 12), n=4, d_s=0.25, d_t=0.625)    # 10 * 0.25 = 2.5 -> 2; 4 * 0.625 = 2.5 -> 2
    cases["box_t12_h12_w16_threshold_1_5"] = dict(kind="box", shape=(12, 12, 16), n=4, d_s=0.25, d_t=0.25)   # 6 * 0.25 = 1.5 -> 2 (half to even)
    cases["box_t6_h12_w12_threshold_1_5_and_2_5"] = dict(kind="box", shape=(6, 12, 12), n=4, d_s=0.25, d_t=0.5)   # (threshold_t 1.5 -> 2)
    # 1 051 100 bins > GRID_CAP; the box threshold 230 * 0.25 = 57.5 rounds to the even 58
    cases["wrap_box_t5_h460_w457"] = dict(kind="box", shape=(5, 460, 457), n=4, d_s=0.25, d_t=0.5)
    cases["wrap_ideal_t5_h460_w457"] = dict(kind="ideal", shape=(5, 460, 457), n=4, d_s=0.25, d_t=0.5)
    cases["wrap_gaussian_t5_h460_w457"] = dict(kind="gaussian", shape=(5, 460, 457), n=4, d_s=0.25, d_t=0.5)
    return cases


FILTER_CASES = _filter_cases()


def filter_eval(c, wrong=None):
    return freq_filter(*c["shape"], c["kind"], c["n"], c["d_s"], c["d_t"], wrong)


def _box_bins(T, H, d_s, d_t, rnd):
    th, tt = rnd(int(H // 2) * d_s), rnd(T // 2 * d_t)
    return (th, tt) if th and tt else (0, 0)


def filter_wrongs(c):
    """half-up (2.5 -> 3) and half-down (1.5 -> 1) rounding apply where they move a threshold of a non-empty box; exchanged cut-offs where they differ; a zero cut-off
    not answered with zeros where the filter is not a box (the box of these shapes is empty at d = 0.25 too)"""
    T, H, W = c["shape"]
    if c["d_s"] == 0 or c["d_t"] == 0:
        return ("zero_cutoff_not_zeros",) if c["kind"] != "box" else ()
    w = ()
    for name, rnd in (("box_threshold_half_up", _round_half_up), ("box_threshold_half_down", _round_half_down)):
        if c["kind"] == "box" and _box_bins(T, H, c["d_s"], c["d_t"], round) != _box_bins(T, H, c["d_s"], c["d_t"], rnd):
            w += (name,)
    if c["d_s"] != c["d_t"] and T > 1:
        w += ("ds_dt_exchanged",)
    return w


# ----------------------------------------------------------------------------------------------------------------- wrong restatements
MUTANTS = {"moca_step": STEP_WRONGS, "step_windows": WIN_WRONGS, "gather_windows": GATHER_WRONGS, "advance": ADV_WRONGS, "prepare_queue": PREP_WRONGS,
           "base_step": BASE_WRONGS, "mask_sums": ("sum_batch0_only", "last_pixel_dropped"), "sam_select": SAM_WRONGS, "freq_filter": FILTER_WRONGS}

# ----------------------------------------------------------------------------------------------------------------- entry points and refusals
# argument order of every entry point under test (lib.SIGNATURES without the stream); "*name" = a pointer
ENTRY = {
    "moca_fifo_randn_f32": "*state *out n",
    "moca_fifo_gather_windows_f32": "*state *queue *x *anchor *win_start nW reps C Q f HW",
    "moca_sam_select_masks_f32": "*cand *cand_off *ncand *t_rows *eff *eff_idx nW f HW",
    "moca_fifo_advance_f32": "*state *queue *newframe *emitted n_slots emit_frame *mask *mask_sums C Q HW",
    "moca_fifo_prepare_queue_f32": "*z *noise *queue *coef_z *coef_noise *frame_idx BC Tz Q HW",
    "moca_base_set_timestep": "*state *table S *rows n",
    "moca_base_ddim_step_f32": "*state *x *eps_c *eps_u *noise *pred_x0 *coef S cfg_scale use_scale n",
    "moca_mask_frame_sums_f32": "*mask *sums frames HW",
    "moca_freq_filter_f32": "*lpf T H W type n d_s d_t",
    "moca_fifo_ddim_step_f32": "*sample *eps *noise *momentum *x_prev *pred_x0 *coef *mask *cond *mask_index *enh *ws B C F Fm HW beta one_minus_beta gamma one_minus_gamma",
    # moca_fifo_step_params (include/moca_hip.h), passed by pointer
    "moca_fifo_step_windows_f32": "*state *x *eps_c *eps_u *noise *momentum *queue *x_prev *pred_x0 *coef *win_start *mask *mask_sums *mask_frame *enh "
                                  "*cond *sam_eff *sam_idx cfg_scale beta one_minus_beta gamma one_minus_gamma nW C Q f HW wb_from",
}
ENTRY = {k: v.split() for k, v in ENTRY.items()}
PTR = True                                 # "a valid pointer": a fake address on the CPU, a zero-filled 64 KiB buffer on the GPU


def _entry_defaults(entry, **kw):
    d = {a.lstrip("*"): (PTR if a.startswith("*") else 2) for a in ENTRY[entry]}
    d.update(kw)
    return d


_W = dict(eps_u=None, mask=None, mask_sums=None, mask_frame=None, enh=None, cond=None, sam_eff=None, sam_idx=None, cfg_scale=1.0, beta=0.9,
          one_minus_beta=0.1, gamma=0.5, one_minus_gamma=0.5, wb_from=1, Q=3)
_MASKED = dict(mask=PTR, mask_sums=PTR, mask_frame=PTR, enh=PTR)
# entry -> (the accepted argument set, [(what the call trips, overrides: one guard clause each)]); every accepted set is tiny: all index
# buffers may be zero and no product of its sizes exceeds 64 KiB of any element type
REFUSALS = {
    "moca_fifo_randn_f32": (_entry_defaults("moca_fifo_randn_f32", n=5), [("state", dict(state=None)), ("out", dict(out=None)), ("n", dict(n=0))]),
    "moca_fifo_gather_windows_f32": (_entry_defaults("moca_fifo_gather_windows_f32", Q=4), [
        ("state", dict(state=None)), ("queue", dict(queue=None)), ("C", dict(C=0)), ("Q", dict(Q=0, x=None, nW=0)), ("HW", dict(HW=0)),
        ("win_start", dict(win_start=None)), ("nW", dict(nW=0)), ("reps", dict(reps=0)), ("f", dict(f=0)), ("f > Q", dict(f=5)),
        ("neither x nor anchor", dict(x=None, anchor=None, nW=0))]),
    "moca_sam_select_masks_f32": (_entry_defaults("moca_sam_select_masks_f32"), [(k, {k: None}) for k in ("cand", "cand_off", "ncand", "t_rows", "eff", "eff_idx")]
                                  + [(k, {k: 0}) for k in ("nW", "f", "HW")]),
    "moca_fifo_advance_f32": (_entry_defaults("moca_fifo_advance_f32", emit_frame=1), [
        ("state", dict(state=None)), ("queue", dict(queue=None)), ("newframe", dict(newframe=None)), ("C", dict(C=0)), ("Q", dict(Q=0)),
        ("HW", dict(HW=0)), ("emit_frame < 0", dict(emit_frame=-1)), ("emit_frame >= Q", dict(emit_frame=2)), ("n_slots", dict(n_slots=0)),
        ("mask without sums", dict(mask_sums=None))]),
    "moca_fifo_prepare_queue_f32": (_entry_defaults("moca_fifo_prepare_queue_f32"),
                                    [(k, {k: None}) for k in ("z", "noise", "queue", "coef_z", "coef_noise", "frame_idx")] + [(k, {k: 0}) for k in ("BC", "Tz", "Q", "HW")]),
    "moca_base_set_timestep": (_entry_defaults("moca_base_set_timestep"), [("state", dict(state=None)), ("table", dict(table=None)), ("rows", dict(rows=None)),
                                                                           ("S", dict(S=0)), ("n", dict(n=0))]),
    "moca_base_ddim_step_f32": (_entry_defaults("moca_base_ddim_step_f32", cfg_scale=1.0, use_scale=1),
                                [(k, {k: None}) for k in ("state", "x", "eps_c", "noise", "coef")] + [("S", dict(S=0)), ("n", dict(n=0))]),
    "moca_mask_frame_sums_f32": (_entry_defaults("moca_mask_frame_sums_f32"), [("mask", dict(mask=None)), ("sums", dict(sums=None)), ("frames", dict(frames=0)), ("HW", dict(HW=0))]),
    "moca_freq_filter_f32": (_entry_defaults("moca_freq_filter_f32", type=3, n=4, d_s=0.25, d_t=0.25),
                             [("lpf", dict(lpf=None)), ("T", dict(T=0)), ("H", dict(H=0)), ("W", dict(W=0)), ("type < 0", dict(type=-1)), ("type > 3", dict(type=4))]),
    "moca_fifo_ddim_step_f32": (_entry_defaults("moca_fifo_ddim_step_f32", beta=0.9, one_minus_beta=0.1, gamma=0.5, one_minus_gamma=0.5),
                                [(k, {k: None}) for k in ("sample", "eps", "noise", "momentum", "x_prev", "pred_x0", "coef")] + [(k, {k: 0}) for k in ("B", "C", "F", "HW")]
                                + [("Fm", dict(Fm=0)), ("mask_index", dict(mask_index=None)), ("enh", dict(enh=None)), ("ws", dict(ws=None))]),
    "moca_fifo_step_windows_f32": (_entry_defaults("moca_fifo_step_windows_f32", **_W), [(k, {k: None}) for k in ("state", "x", "eps_c", "noise", "momentum", "coef", "win_start")]
                                   + [(k, {k: 0}) for k in ("nW", "C", "f", "HW")] + [
        ("wb_from", dict(wb_from=-1)), ("queue with Q < f", dict(Q=1)), ("mask without sums", dict(_MASKED, mask_sums=None)),
        ("mask without frames", dict(_MASKED, mask_frame=None)), ("mask without enh", dict(_MASKED, enh=None)),
        ("mask with Q <= 0", dict(_MASKED, queue=None, Q=0)), ("sam_eff without sam_idx", dict(sam_eff=PTR)),
        ("both branches", dict(_MASKED, sam_eff=PTR, sam_idx=PTR)), ("no output", dict(queue=None, x_prev=None, pred_x0=None))]),
}
# further accepted sets next to the refusals above: the variants whose refusals differ from the first set in more than the tripped clause
ACCEPTED_ALSO = {
    "moca_fifo_gather_windows_f32": [dict(x=None, nW=0, Q=1)],
    "moca_fifo_step_windows_f32": [dict(_MASKED), dict(_MASKED, queue=None), dict(sam_eff=PTR, sam_idx=PTR), dict(queue=None, x_prev=None)],
    "moca_fifo_advance_f32": [dict(emitted=None, n_slots=0), dict(mask=None, mask_sums=None)],
    "moca_fifo_ddim_step_f32": [dict(mask=None, Fm=0, mask_index=None, enh=None, ws=None)],
}


def call(lib_mod, entry, args, pointer):
    """launch `entry` with the argument dict `args`; pointer(name, value) maps a pointer argument to an address or None"""
    import ctypes as C
    lib = lib_mod.load()
    vals = [pointer(a[1:], args[a[1:]]) if a.startswith("*") else args[a] for a in ENTRY[entry]]
    if entry == "moca_fifo_step_windows_f32":
        p = lib_mod.FifoStepParams()
        for a, v in zip(ENTRY[entry], vals):
            setattr(p, a.lstrip("*"), v)
        return lib.moca_fifo_step_windows_f32(C.byref(p), args.get("stream"))
    return getattr(lib, entry)(*vals, args.get("stream"))


# ----------------------------------------------------------------------------------------------------------------- threshold arithmetic
def iou_ratio_values():
    """every ratio inter / union a pair of masks over at most 12 united pixels can have: 90 (inter, union) pairs (union 0 counts as 1 = 1/1)"""
    return [(i, u) for u in range(1, 13) for i in range(0, u + 1)]
