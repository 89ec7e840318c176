"""CPU: the restatements, case tables and standards of tests/test_step_kernels_gpu.py check themselves (tests/step_kernels_ref.py).

  test_restatements_equal_the_oracle ........ the fp32 restatements of the MoCA step (mask branch, segmentation branch, neither) and of
                                              the base DDIM step equal oracle.sampler_oracle.ddim_step / p_sample_ddim bit for bit on
                                              every case those functions can express (one video per call with masks, mask frame = frame)
  test_fp32_stays_near_float64 .............. every fp32 restatement is the float64 one to fp32 rounding; prints the worst ratio per family
  test_cases_tell_errors .................... every case tells every wrong restatement that applies to it, by torch.equal; every wrong
                                              restatement applies to at least one case
  test_sam_select_is_the_host_bookkeeping ... the scripted segmentation windows: restatement == DDIMSampler.select_sam_masks
  test_refusals_without_a_gpu ............... one call per guard clause of every entry point returns MOCA_E_BADARG before any launch
  test_iou_threshold_is_decidable ........... the kernel's sequential fp32 IoU mean and torch.tensor(ious).mean() decide `< 0.5` alike for
                                              all 737 190 ordered combinations of 1 to 3 ratios i / u, u <= 12
  test_ideal_filter_cases_are_decidable ..... no ideal-filter case has a bin within 1e-9 of its cut-off unless equal in double arithmetic
  test_philox_variants, test_case_tables_name_the_edges, test_new_gpu_tests_are_in_the_ledger"""
import types
from fractions import Fraction

import numpy as np
import torch

import small_kernels_ref as SR
import step_kernels_ref as R

F32, F64 = torch.float32, torch.float64


def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _schedule():
    from oracle import sampler_oracle as SO
    return SO, SO.make_schedule(SO.ddpm_buffers(), 16, 1.0)


def _coef6(sch, indices):
    """the six coefficients per frame as the reference's 0-dim fp32 tensors give them (ddim.py:409-428)"""
    rows = []
    for index in indices:
        a_t, a_prev, sig = (torch.full((1,), float(sch[k][index])) for k in ("ddim_alphas", "ddim_alphas_prev", "ddim_sigmas"))
        s1m = torch.full((1,), float(sch["ddim_sqrt_one_minus_alphas"][index]))
        t = torch.tensor(int(sch["ddim_timesteps"][index]))
        rows.append(torch.cat([torch.sqrt(a_t), torch.sqrt(a_prev), sig, s1m, torch.sqrt(1. - a_prev - sig ** 2), (2 * (1.0 - t / 1000.0)).reshape(1)]))
    return torch.stack(rows)


def test_restatements_equal_the_oracle():
    SO, sch = _schedule()
    n = 0
    idx_all = [0, 0, 2, 3, 4, 7, 9, 15]
    for name, c in R.STEP_CASES.items():
        if c["mask"] and c["B"] != 1:
            continue                                      # (the oracle's mask expand wants one video per call)
        t = R.step_inputs(c)
        B, Cc, F, Fm, HW = c["B"], c["C"], c["F"], c["Fm"], c["HW"]
        indices = idx_all[:F]
        ts = [torch.tensor(int(sch["ddim_timesteps"][i])) for i in indices]
        coef = _coef6(sch, indices)
        mi = torch.tensor([j if (c["mask"] and j < Fm) else -1 for j in range(F)], dtype=torch.int32)
        enh = torch.tensor([1.5 if int(x) <= 300 else 1.0 for x in ts])
        v5 = lambda a: a.reshape(B, Cc, F, 1, HW)
        mom = v5(t["mom"]).clone()
        xp_o, p0_o = SO.ddim_step(sch, v5(t["sample"]), v5(t["eps"]), indices, None if t["cond"] is None else t["cond"].reshape(B, Cc, 1, 1, HW), ts,
                                  [v5(t["noise"])[:, :, [j]] for j in range(F)], mom,
                                  davis_masks=t["mask"].reshape(B, 1, Fm, 1, HW) if c["mask"] else None, reference_index_quirk=False) \
            if (t["cond"] is not None or not c["mask"]) else (None, None)
        if xp_o is None:
            continue                                      # (the reference multiplies cond_image: there is no "no condition image" with masks)
        xp, p0, m = R.moca_step(t["sample"], t["eps"], t["noise"], t["mom"], coef, t["mask"], t["cond"], mi, enh, F32, **R.STEP_ARGS)
        assert torch.equal(v5(xp), xp_o) and torch.equal(v5(p0), p0_o) and torch.equal(v5(m), mom), name
        n += 1
    assert n >= 4
    # the segmentation branch and the windows restatement: one window, no ring, scripted candidates
    for name in ("hw260_sum_exactly_80_percent_no_reset_one_more_resets", "hw260_first_frame_without_detection", "hw65_basic"):
        HW, cands, tsw = R.sam_script(name)
        f, Cc = len(tsw), 3
        g = R.gen(77)
        x, e_c, e_u, nz, mom0 = (torch.randn(1, Cc, f, HW, generator=g) for _ in range(5))
        cond = torch.rand(Cc, HW, generator=g) + 0.25
        indices = [{100: 1, 300: 4, 301: 5}[int(t)] for t in tsw]              # ddim_timesteps 67, 266, 333: the same side of 300
        ts = [torch.tensor(int(sch["ddim_timesteps"][i])) for i in indices]
        eff, idx = R.sam_select(cands, np.asarray([int(t) for t in ts]), HW)
        coef = _coef6(sch, indices)[None]
        got = R.step_windows(x, e_c, e_u, nz, mom0, coef, None, 0, [0], 0, 12.0, enh=torch.ones(1, f), cond=cond, sam_eff=eff[None],
                             sam_idx=torch.from_numpy(idx)[None], dtype=F32, **R.STEP_ARGS)
        v5 = lambda a: a.reshape(1, Cc, f, 1, HW)
        mom = v5(mom0).clone()
        eps = R.guidance(e_c, e_u, 12.0, F32)
        assert torch.equal(eps, e_u + 12.0 * (e_c - e_u))
        xp_o, p0_o = SO.ddim_step(sch, v5(x), v5(eps), indices, cond.reshape(1, Cc, 1, 1, HW), ts, [v5(nz)[:, :, [j]] for j in range(f)], mom,
                                  sam_masks=[None if c is None else c.reshape(-1, 1, HW) for c in cands], reference_index_quirk=False)
        assert torch.equal(v5(got[0]), xp_o) and torch.equal(v5(got[1]), p0_o) and torch.equal(v5(got[2]), mom), name
    # base step: every schedule row, both use_scale settings
    S = 16
    coef8 = torch.zeros(S, 8)
    for i in range(S):
        coef8[i, :5] = _coef6(sch, [i])[0, :5]
        coef8[i, 5], coef8[i, 6] = float(sch["ddim_scale_arr"][i]), float(sch["ddim_scale_arr_prev"][i])
    g = R.gen(78)
    x, e_c, e_u, nz = (torch.randn(2, 3, 4, 5, 7, generator=g) for _ in range(4))
    for it in (0, 7, 15, 16, 35):
        for use_scale in (0, 1):
            xp, p0 = R.base_step(x, e_c, e_u, nz, coef8, it, S, 7.5, use_scale, F32)
            xp_o, p0_o = SO.p_sample_ddim(sch, x, e_c, e_u, 7.5, S - 1 - it % S, nz, use_scale=bool(use_scale))
            assert torch.equal(xp, xp_o) and torch.equal(p0, p0_o), (it, use_scale)


def test_sam_select_is_the_host_bookkeeping():
    from moca_video_amd.sampler import DDIMSampler
    s = DDIMSampler(types.SimpleNamespace(num_timesteps=1000))
    for name in R.SAM_SCRIPTS:
        HW, cands, ts = R.sam_script(name)
        eff, idx = R.sam_select(cands, ts, HW)
        eff_h, idx_h = s.select_sam_masks([None if c is None else c.reshape(-1, 1, HW) for c in cands], ts, 1, HW, "cpu")
        assert np.array_equal(idx, idx_h), name
        for i in range(len(ts)):
            assert torch.equal(eff[i], eff_h[i] if idx[i] >= 0 else torch.full((HW,), R.SAM_SENTINEL)), (name, i)
    for seed in (1, 2):                                     # and the windows the segmentation branch of the step cases is fed with
        for cands, ts in R.sam_windows_for(3, 8, 65, seed):
            eff, idx = R.sam_select(cands, ts, 65)
            eff_h, idx_h = s.select_sam_masks([None if c is None else c.reshape(-1, 1, 65) for c in cands], ts, 1, 65, "cpu")
            assert np.array_equal(idx, idx_h) and all(torch.equal(eff[i], eff_h[i]) for i in range(8) if idx[i] >= 0)
            assert (idx < 0).any() and (idx >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- fp32 against float64
def _near(f32, f64, what, worst):
    """each fp32 operation rounds by half an ulp of its own result; the chains here are at most ~12 operations per frame, the division
    by sqrt(a_t) >= 0.3 amplifies by 3.3 at most and a frame feeds the next one through the momentum term with a factor
    cf5 (1 - beta) < 0.13: 64 ulps of the largest magnitude is far above what a right fp32 evaluation needs, far below any wrong term"""
    for a, b in zip(f32, f64):
        if a is None:
            continue
        assert a.dtype == F32 and b.dtype == F64
        r = ((a.double() - b).abs().max() / (2.0 ** -23 * b.abs().max())).item()
        worst[what] = max(worst.get(what, 0.0), r)
        assert r <= 64, f"{what}: fp32 is {r:.1f} ulps of max|ref| from float64"


def test_fp32_stays_near_float64():
    worst = {}
    for name, c in R.STEP_CASES.items():
        t = R.step_inputs(c)
        _near(R.step_eval(c, F32, t=t), R.step_eval(c, F64, t=t), "moca_step", worst)
        if c["mask"]:
            assert torch.equal(R.mask_batch_sums(t["mask"], F32).double(), R.mask_batch_sums(t["mask"], F64))
    for name, c in R.WIN_CASES.items():
        t = R.win_inputs(c)
        a, b = R.win_eval(c, F32, t=t), R.win_eval(c, F64, t=t)
        _near([a[k] for k in a], [b[k] for k in a], "step_windows", worst)
    for name, c in R.PREP_CASES.items():
        t = R.prep_inputs(c)
        _near([R.prep_eval(c, F32, t=t)], [R.prep_eval(c, F64, t=t)], "prepare_queue", worst)
    for name, c in R.BASE_CASES.items():
        t = R.base_inputs(c)
        _near(R.base_eval(c, F32, t=t), R.base_eval(c, F64, t=t), "base_step", worst)
    for HW in R.HWS:
        m = R.sums_inputs(HW, 6000 + HW)
        assert torch.equal(R.mask_frame_sums(m, F32).double(), R.mask_frame_sums(m, F64)), "mask sums are exact in fp32"
    print("\nworst |fp32 - fp64| / (2^-23 max|fp64|): " + ", ".join("%s %.2f" % kv for kv in worst.items()))


# ---------------------------------------------------------------------------------------------------------------- mutants
def test_cases_tell_errors():
    seen = set()

    def tell(family, table, wrongs, ev):
        for name, c in table.items():
            right = ev(c, None)
            for w in wrongs(c):
                assert w in R.MUTANTS[family], (family, w)
                seen.add((family, w))
                assert not _same(right, ev(c, w)), f"{family} {name}: the wrong restatement `{w}` gives the right result"

    memo = {}

    def inputs(fn, c):
        if id(c) not in memo:
            memo.clear()
            memo[id(c)] = fn(c)
        return memo[id(c)]

    tell("moca_step", R.STEP_CASES, R.step_wrongs, lambda c, w: R.step_eval(c, F32, w, inputs(R.step_inputs, c)))
    tell("step_windows", R.WIN_CASES, R.win_wrongs, lambda c, w: R.win_eval(c, F32, w, inputs(R.win_inputs, c)))
    tell("gather_windows", R.GATHER_CASES, R.gather_wrongs, lambda c, w: R.gather_eval(c, F32, w)[1:])
    tell("advance", R.ADV_CASES, R.adv_wrongs, lambda c, w: R.adv_eval(c, w, inputs(R.adv_inputs, c)))
    tell("prepare_queue", R.PREP_CASES, R.prep_wrongs, lambda c, w: R.prep_eval(c, F32, w, inputs(R.prep_inputs, c)))
    tell("base_step", R.BASE_CASES, R.base_wrongs, lambda c, w: R.base_eval(c, F32, w, inputs(R.base_inputs, c)))
    tell("freq_filter", R.FILTER_CASES, R.filter_wrongs, lambda c, w: R.filter_eval(c, w))
    tell("sam_select", {n: n for n in R.SAM_SCRIPTS}, lambda n: R.SAM_TELLS[n],
         lambda n, w: (lambda HW, cands, ts: R.sam_select(cands, ts, HW, w))(*R.sam_script(n)))
    for name, c in R.TIMESTEP_ROW_CASES.items():
        if c["S"] > 1:
            assert R.schedule_row(c["iter"], c["S"]) != R.schedule_row(c["iter"], c["S"], "row_iter_mod_s"), name
    for HW in R.HWS:
        m = R.sums_inputs(HW, 6000 + HW)
        assert not torch.equal(R.mask_frame_sums(m, F32), R.mask_frame_sums(m, F32, "last_pixel_dropped")), HW
        seen.add(("mask_sums", "last_pixel_dropped"))
    for name, c in R.STEP_CASES.items():
        if c["mask"] and c["B"] == 2:
            m = R.step_inputs(c)["mask"]
            assert not torch.equal(R.mask_batch_sums(m, F32), R.mask_batch_sums(m, F32, "sum_batch0_only")), name
            seen.add(("mask_sums", "sum_batch0_only"))
    missing = {(f, w) for f, ws in R.MUTANTS.items() for w in ws} - seen
    assert not missing, f"wrong restatements no case applies: {missing}"
    assert set(R.SAM_TELLS) == set(R.SAM_SCRIPTS)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _fake(name, v):
    return None if v is None else 0x10000


def test_refusals_without_a_gpu():
    """every call differs from its entry's accepted set (fake 4 KiB-aligned pointers; the GPU file launches the accepted sets) in what
    one guard clause refuses and returns MOCA_E_BADARG before any launch"""
    from moca_video_amd import lib
    assert set(R.REFUSALS) == set(R.ENTRY)
    n = 0
    for entry, (ok, bad) in R.REFUSALS.items():
        assert len(lib.SIGNATURES[entry][1]) == (2 if entry == "moca_fifo_step_windows_f32" else len(R.ENTRY[entry]) + 1), entry
        labels = [b[0] for b in bad]
        assert len(set(labels)) == len(labels), entry
        for label, over in bad:
            assert set(over) <= set(ok), (entry, label)
            assert R.call(lib, entry, dict(ok, **over), _fake) == -1, f"{entry}: `{label}` is not refused"
            n += 1
    assert lib.load().moca_fifo_step_windows_f32(None, None) == -1
    assert n >= 100
    # no entry point has more refusing statements than calls above
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moca_video_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in ("fifo.hip", "sampler.hip", "freeinit.hip")}
    for entry, (ok, bad) in R.REFUSALS.items():
        body = next(s[s.index('extern "C" int %s(' % entry):] for s in src.values() if 'extern "C" int %s(' % entry in s)
        assert 1 <= body[:body.index("hipLaunchKernelGGL")].count("return MOCA_E_BADARG") <= len(bad), entry


# ---------------------------------------------------------------------------------------------------------------- threshold arithmetic
def test_iou_threshold_is_decidable():
    vals = R.iou_ratio_values()
    assert len(vals) == 90
    r = np.asarray([np.float32(i) / np.float32(u) for i, u in vals], np.float32)
    total = 0
    for k in (1, 2, 3):
        grid = np.stack(np.meshgrid(*([r] * k), indexing="ij"), -1).reshape(-1, k)
        acc = np.zeros(len(grid), np.float32)
        for j in range(k):
            acc = (acc + grid[:, j]).astype(np.float32)                       # the kernel: sequential fp32 sum ...
        kern = (acc / np.float32(k)).astype(np.float32)                        # ... and one fp32 division
        ref = torch.from_numpy(grid).mean(1).numpy()
        assert np.array_equal(kern < 0.5, ref < 0.5), k
        for n in np.flatnonzero(kern == 0.5):                                  # an fp32 mean of exactly 0.5 is an exact mean of 0.5
            pairs = [vals[a] for a in np.unravel_index(n, (90,) * k)]
            assert sum(Fraction(i, u) for i, u in pairs) == Fraction(k, 2), pairs
        # the reference's own call, literally, where the decision is closest
        for n in np.flatnonzero(np.abs(kern - 0.5) < 1e-6)[:2000]:
            assert (torch.tensor([float(v) for v in grid[n]]).mean().item() < 0.5) == bool(kern[n] < 0.5)
        total += len(grid)
    assert total == 737190
    assert R.iou_mean_f32([0.25, 0.5, 0.75]) == 0.5 and R.iou_mean_f32([np.float32(1) / np.float32(3)] * 3) < 0.5


def test_ideal_filter_cases_are_decidable():
    n = 0
    for name, c in R.FILTER_CASES.items():
        if c["kind"] == "ideal" and c["d_s"] and c["d_t"]:
            assert R.ideal_margin(*c["shape"], c["d_s"], c["d_t"]) > 1e-9, name
            n += 1
    assert n >= 5
    # the box thresholds that land on .5 round to even
    c = R.FILTER_CASES
    assert round(5 * 0.5) == 2 and round(10 * 0.25) == 2 and round(6 * 0.25) == 2 and round(230 * 0.25) == 58
    for name in ("box_t4_h10_w12_threshold_2_5", "box_t8_h20_w12_threshold_2_5", "box_t12_h12_w16_threshold_1_5"):
        T, H, W = c[name]["shape"]
        th = round(int(H // 2) * c[name]["d_s"])
        assert int(H // 2) * c[name]["d_s"] % 1 == 0.5 and th == 2, name
    assert "box_threshold_half_up" in R.filter_wrongs(c["box_t8_h20_w12_threshold_2_5"]) and "box_threshold_half_down" in R.filter_wrongs(c["box_t12_h12_w16_threshold_1_5"])
    assert R.filter_eval(c["box_t8_h20_w12_threshold_2_5"]).sum() == 4 * 4 * 4
    for name, cc in c.items():                               # a zero cut-off is zeros
        if cc["d_s"] == 0 or cc["d_t"] == 0:
            assert not R.filter_eval(cc).any(), name


def test_philox_variants():
    """the reference noise of the GPU file: the fp32-angle variant differs from the plain float64 one by the angle's rounding only"""
    for n in (1, 5, 1023):
        a = R.philox_numpy(R.RANDN_SEED, 3, n)
        b, r = R.philox_numpy(R.RANDN_SEED, 3, n, f32_angle=True, with_r=True)
        assert a.shape == b.shape == r.shape == (n,)
        # |d angle| <= half an fp32 ulp of an angle in [4, 8) + 2 pi |1 - fp32(2 pi) / 2 pi|, |d z| <= r |d angle|
        assert np.abs(a - b).max() <= (2.0 ** -22 + 1.8e-7) * r.max() and (r > 0).all()
    assert not np.array_equal(R.philox_numpy(R.RANDN_SEED, 0, 16), R.philox_numpy(R.RANDN_SEED, 1, 16))
    assert not np.array_equal(R.philox_numpy(R.RANDN_SEED, 0, 16), R.philox_numpy(R.RANDN_SEED ^ 1, 0, 16))
    assert not np.array_equal(R.philox_numpy(R.RANDN_SEED, 0, 16), R.philox_numpy(R.RANDN_SEED ^ (1 << 32), 0, 16))
    assert R.RANDN_BOUND == 2 * R.RANDN_MEASURED and "%.3f" % R.RANDN_MEASURED in R.__doc__


def test_case_tables_name_the_edges():
    assert R.GRID_CAP is SR.GRID_CAP and R.WRAP == SR.GRID_CAP + 300 and R.edge_items is SR.edge_items
    for table in (R.STEP_CASES, R.WIN_CASES, R.GATHER_CASES, R.ADV_CASES, R.PREP_CASES, R.BASE_CASES, R.TIMESTEP_ROW_CASES, R.RANDN_CASES, R.FILTER_CASES):
        assert sum(n.startswith("wrap") for n in table) >= 1 and any(not n.startswith("wrap") for n in table)
    work = {"step": lambda c: c["B"] * c["C"] * c["HW"], "win": lambda c: len(c["starts"]) * c["C"] * c["HW"],
            "gather": lambda c: len(c["starts"]) * c["C"] * c["f"] * c["HW"], "adv": lambda c: c["C"] * c["HW"],
            "prep": lambda c: c["BC"] * c["Q"] * c["HW"], "base": lambda c: c["n"]}
    for key, table in (("step", R.STEP_CASES), ("win", R.WIN_CASES), ("gather", R.GATHER_CASES), ("adv", R.ADV_CASES), ("prep", R.PREP_CASES), ("base", R.BASE_CASES)):
        for name, c in table.items():
            assert (work[key](c) > R.GRID_CAP) == name.startswith("wrap"), name
        small = [c for n, c in table.items() if not n.startswith("wrap")]
        if key != "base":
            assert {c["HW"] for c in small} >= set(R.HWS), key
            assert {c.get("C", 1) for c in small} >= ({1, 3, 4} if key not in ("prep",) else {1})
    assert R.RANDN_CASES["wrap_4_caps_plus_5"] == 4 * R.GRID_CAP + 5 and {R.RANDN_CASES[k] % 4 for k in R.RANDN_CASES} == {0, 1, 2, 3}
    assert {c["B"] for c in R.STEP_CASES.values()} == {1, 2} and {c["F"] for c in R.STEP_CASES.values()} == {1, 2, 8}
    assert all(c["Fm"] != c["F"] for c in R.STEP_CASES.values())
    assert {(c["Q"] - c["f"]) for c in R.WIN_CASES.values()} >= {0, 1, 12} and {c["wb_from"] * 2 // c["f"] for c in R.WIN_CASES.values()} == {0, 1, 2}
    for c in R.WIN_CASES.values():
        if c["wb_from"] == 0 and c["queue"]:                 # write-back of whole windows: they must be disjoint
            fr = [(c["head"] + s + j) % c["Q"] for s in c["starts"] for j in range(c["f"])]
            assert len(set(fr)) == len(fr)
    assert {c["emit_frame"] for c in R.ADV_CASES.values()} >= {0, 4, 19} and {c["iter"] for c in R.ADV_CASES.values() if c["n_slots"] == 3} >= {0, 2, 3, 7}
    assert {c["BC"] for c in R.PREP_CASES.values()} == {1, 8} and {c["Tz"] for c in R.PREP_CASES.values()} == {1, 3, 16}
    assert all(c["Tz"] != c["Q"] for c in R.PREP_CASES.values())
    assert {(c["S"], c["iter"]) for c in R.BASE_CASES.values()} >= {(1, 0), (6, 0), (6, 5), (6, 6), (6, 15)}
    assert {c["shape"] for c in R.FILTER_CASES.values()} >= {(1, 1, 1), (3, 5, 7), (16, 10, 12), (4, 20, 6)}
    assert {HW for HW, _ in R.SAM_SCRIPTS.values()} == {1, 65, 260}
    for name, c in R.FILTER_CASES.items():
        assert (np.prod(c["shape"]) > R.GRID_CAP) == name.startswith("wrap"), name
    assert "box_threshold_half_down" in R.filter_wrongs(R.FILTER_CASES["wrap_box_t5_h460_w457"])


def test_new_gpu_tests_are_in_the_ledger():
    import test_step_kernels_gpu as G
    want = {"moca_fifo_ddim_step_f32": "test_moca_step", "moca_fifo_step_windows_f32": "test_step_windows", "moca_fifo_gather_windows_f32": "test_gather_windows",
            "moca_fifo_advance_f32": "test_advance", "moca_fifo_prepare_queue_f32": "test_prepare_queue", "moca_base_set_timestep": "test_base_set_timestep",
            "moca_base_ddim_step_f32": "test_base_step", "moca_mask_frame_sums_f32": "test_mask_frame_sums", "moca_sam_select_masks_f32": "test_sam_select_scripted",
            "moca_fifo_randn_f32": "test_randn", "moca_freq_filter_f32": "test_freq_filter"}
    assert set(want) == set(R.ENTRY)
    for sym, fn in want.items():
        assert "test_step_kernels_gpu::" + fn in SR.LEDGER[sym], sym
        assert callable(getattr(G, fn))
        assert len(SR.LEDGER[sym]) >= 2, "the earlier entries stay"
