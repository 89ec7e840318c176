"""CPU: the case tables and the references of tests/test_gemm_fused_gpu.py check themselves (tests/gemm_fused_ref.py).

  test_routes_without_a_device ... for every case of every table the host queries, under the case's knobs and on operands laid out as
                                   the GPU file lays them out (lda = K + 8, ldo = N + 8, ld_ln = N + 16, ldr = N + 24, the weight gap),
                                   answer the route and the `_ok` values the GPU test will assert; the refused case answers 0 and
                                   moca_gemm_f16 returns the bad-argument code without a launch
  test_wrong_restatements ........ at every case's shape and seed every wrong float64 restatement that applies is at least 10 x the
                                   bound away from the right one under the measure the GPU file uses (per 64-row block; per slice and
                                   per pixel-within-tile; per accumulator).  One restatement cannot be: see VAR_N_MINUS_1.
  test_slack_stays_below_tol ..... the "twice plain fp32" slack of the large-row-mean blocks stays below TOL16 for the chosen inputs
  test_tattn_restatements_agree .. the fold's projection restated on the folded fp16 operands and on the unfolded weights: equal within
                                   TOL16 in the ordinary regime, not in the peaked one (why the GPU file uses the former)
  test_tables_hold_the_edges ..... the tables contain the shapes, strides and branch counts the suite is about
  test_ledger .................... the ledger of tests/small_kernels_ref.py names the new tests, the earlier entries stay

VAR_N_MINUS_1: a variance over N - 1 moves ln_out by 1 / (2 (N - 1)) = 1.6e-3 of itself at N = 320, the only width the store loop has:
half of TOL16, so no per-block comparison of ln_out at that bound can tell it, let alone at 10 x.  What can is the row power of a
unit-gamma, zero-beta row -- mean of ln_out^2 = var / (var + eps), which that error moves by 1 / N = 3.1e-3 -- bounded by TOL_ROWPOWER =
2^-10 + 2^-13 (gemm_fused_ref.py: one fp16 rounding per stored value); the restatement must exceed twice that bound there, and on ln_out
itself it must be the 0.4 / (N - 1) .. 1 / (N - 1) that the arithmetic gives."""
import ctypes

import pytest
import torch

import gemm_edges_ref as R
import gemm_fused_ref as FR
import small_kernels_ref as SR
from gemm_edges_ref import TOL16
from moca_video_amd import lib as L
from moca_video_amd import ops


@pytest.mark.parametrize("sec", list(FR.SECTIONS))
def test_routes_without_a_device(sec):
    seen = set()
    for c in FR.SECTIONS[sec]():
        saved = {k: L.set_tuning(k, v) for k, v in FR.case_knobs(c).items()}
        try:
            if sec == "F":
                t = FR.tattn_build(c, FR.tattn_operands(c), "cpu")
                ok = {"tattn_ok": ops.gemm_tattn_ok(t["a"], t["pw"], **t["kw"])}
            else:
                t = FR.build(c, FR.operands(c), "cpu")
                ok = FR.feature_ok(t)
            route = ops.gemm_route(t["a"], t["pw"], t["out"], **t["kw"])
            assert route == FR.ROUTE_ID[c["route"]], f"{FR.case_id(c)}: runs on route {route}"
            if c["route"] == "refused":
                assert ok == {"tattn_ok": False}, FR.case_id(c)
                p = ops._gemm_params(t["a"], t["pw"], t["out"], **t["kw"])
                assert L.load().moca_gemm_f16(ctypes.byref(p), None) == -1, "MOCA_E_BADARG, before any launch"
            else:
                assert ok and all(ok.values()), f"{FR.case_id(c)}: {ok}"
            if c.get("under"):                         # without the second source the persistent kernel takes the call
                plain = {k: v for k, v in t["kw"].items() if k != "a2"}
                a = torch.empty(1, c["K"] + 8, dtype=torch.float16)[:, :c["K"]]
                assert ops.gemm_route(a, t["pw"], t["out"], **plain) == R.ROUTE_ID[c["under"]]
            seen.add(c["route"])
        finally:
            for k, v in saved.items():
                L.set_tuning(k, v)
    want = {"A": {"w80w"}, "B": set(FR.FOLD_ROUTES) | set(R.PERSISTENT), "C": {"w80", "w80w"}, "D": {"w80", "w80w", "ws"},
            "E": set(FR.GSTAT_ROUTES), "F": {"tattn", "refused"}}[sec]
    assert seen == want, f"section {sec} reaches {seen}"


def _distance(c, right, bad):
    """the GPU file's measure between two restatements, in units of its bound"""
    if c["sec"] == "F":
        return FR.tattn_errors(bad["out"], right["out"], c) / TOL16
    d = R.block_errors(bad["out"], right["out"]).max().item() / TOL16
    if right.get("ln") is not None:
        d = max(d, R.block_errors(bad["ln"], right["ln"]).max().item() / TOL16)
    return d


@pytest.mark.parametrize("sec", list(FR.SECTIONS))
def test_wrong_restatements(sec):
    used = set()
    for c in FR.SECTIONS[sec]():
        if c["route"] == "refused":
            continue
        o = FR.tattn_operands(c) if sec == "F" else FR.operands(c)
        ref = FR.tattn_reference if sec == "F" else FR.reference
        right = ref(c, o)
        for wrong in FR.wrongs_of(c):
            used.add(wrong)
            what = f"{FR.case_id(c)}: the {wrong} restatement"
            if wrong in ("coff_ignored", "seam_to_left_neighbour"):
                d, _ = FR.pair_errors(FR.gstat_expected(c, right["out"], wrong), FR.gstat_expected(c, right["out"]))
                assert d > 10 * FR.TOL_GSTAT, f"{what} is only {d:.1e} away"
                continue
            bad = ref(c, o, wrong)
            if wrong == "var_n_minus_1":               # (see VAR_N_MINUS_1 in the module docstring)
                d = R.block_errors(bad["ln"], right["ln"]).max().item()
                assert 0.4 / (c["N"] - 1) < d < 1.0 / (c["N"] - 1), f"{what}: {d:.2e}"
                if c["ln"] == "unit":
                    power = lambda t: (t.half().double() ** 2).mean(1)
                    dp = (power(bad["ln"]) - power(right["ln"])).abs().min().item()
                    assert dp > 2 * FR.TOL_ROWPOWER, f"{what} moves the row power by only {dp:.1e}"
                continue
            d = _distance(c, right, bad)
            assert d > 10, f"{what} is only {d:.1f} x the bound away"
    assert used >= set(FR.WRONGS[sec]) and len(FR.WRONGS[sec]) >= 2, f"section {sec}: never applied {set(FR.WRONGS[sec]) - used}"


def test_slack_stays_below_tol():
    """the large-row-mean blocks (A: residual offset 40 / 100; B: rows 64 .. 127 with |mean| / std = 100) may exceed TOL16 by twice the
    error of the same formula in fp32 torch: that slack is below TOL16 itself, so it can never be what lets a failure through; and the
    inputs are what the tables promise (the ratio, the constant row, distinct rows)"""
    n = 0
    for c in FR.ln_cases() + FR.fold_cases():
        if not (c["res_offset"] or c["nparts"]):
            continue
        o = FR.operands(c)
        tol, slack = FR.block_tol(c, o, FR.reference(c, o))
        assert slack.max().item() < TOL16, f"{FR.case_id(c)}: slack {slack.max().item():.2e}: lower the offset"
        assert (tol >= TOL16).all()
        n += bool(slack.max() > 0)
        if c["nparts"]:
            x = o["a"].double()
            lo, hi = FR.FOLD_BIG
            ratio = (x[lo:hi].mean(1).abs() / x[lo:hi].std(1)).mean().item()
            assert abs(ratio / (FR.FOLD_BIG_RATIO_GEGLU if c["geglu"] else FR.FOLD_BIG_RATIO) - 1) < 0.1 and x[FR.FOLD_CONST_ROW].std().item() == 0.0, FR.case_id(c)
            others = torch.tensor([m for m in range(c["M"]) if not (lo <= m < hi) and m != FR.FOLD_CONST_ROW][:170])
            mean = x[others].mean(1)
            assert (mean - ((others % 17) - 8)).abs().mean() < 0.5, "every row keeps its own mean (sample noise: <= 3 / sqrt(K) per row)"
    assert n > 100


def test_tables_hold_the_edges():
    ln = FR.ln_cases()
    assert {c["M"] for c in ln} >= {161, 320, 321, 641, 480} and {c["K"] for c in ln} == {64, 192}
    assert {c["div"] for c in ln if c["M"] == 641} == {0, 1, 7, 641} and any(c["alias"] for c in ln)
    assert {c["res_offset"] for c in ln} == {0.0, 40.0, 100.0} and {c["ln"] for c in ln} == {"std", "gamma0", "unit"}
    assert {c["groups"] for c in ln} == {0, 2, 3}
    fold = FR.fold_cases()
    for route in FR.FOLD_ROUTES:
        mine = [c for c in fold if c["route"] == route and not c["geglu"]]
        assert {c["nparts"] for c in mine} == set(FR.FOLD_NPARTS) and {c["M"] for c in mine} == set(R.ROUTES[route]["M"])
        assert {c["N"] for c in mine} == set(R.route_Ns(route)) and {(c["bias"], c["res"], bool(c["div"])) for c in mine} >= {(True, False, False), (False, True, True)}
    assert {c["route"] for c in fold if c["geglu"]} == set(FR.FOLD_GEGLU)
    assert FR.FOLD_ROUTES == ("glds128", "glds160", "g4", "w80", "w80w")
    assert not any(c["geglu"] for c in fold if c["route"].startswith("glds")), "the 256-row kernel has the fold in its plain epilogue only"
    for name in R.PERSISTENT:
        assert {(c["M"], c["N"], c["K"]) for c in fold if c["route"] == name} == {R.PERSISTENT_SHAPE[name]}
    cat = FR.cat_cases()
    assert {(c["K"], c["k1"]) for c in cat if not c["under"]} == set(FR.CAT_KS) and {c["under"] for c in cat} == {None, "sqp", "g4p"}
    assert all(any(c[e] for c in cat if c["route"] == r) for r in ("w80", "w80w") for e in ("rowsum", "colsum", "gstat", "res"))
    wg = FR.wgroup_cases()
    for route in ("w80", "w80w"):
        tm = FR.tile_rows(route)
        assert {(c["groups"], c["M"] // c["groups"]) for c in wg if c["route"] == route} == {(2, tm), (2, 2 * tm), (3, tm), (3, 2 * tm)}
    assert {(c["groups"], c["M"]) for c in wg if c["route"] == "ws"} == {(2, 8192), (3, 8256)} and all(c["gap"] == 64 for c in wg)
    assert all(c["gstat"][0] == c["M"] // c["groups"] for c in wg if c["gstat"]), "gstat_rows == wgroup_rows"
    gs = FR.gstat_cases()
    for route in FR.GSTAT_ROUTES:
        tm = FR.tile_rows(route)
        mine = [c for c in gs if c["route"] == route]
        assert {(c["M"] // c["gstat"][0], c["gstat"][0]) for c in mine} == {(2, tm), (2, 2 * tm), (3, tm), (3, 2 * tm)}
        assert any((c["gstat"][2] + c["N"] - 1) // c["gstat"][1] == 31 for c in mine if c["gstat"][1])
    assert {c["gstat"][1:] for c in gs if c["N"] == 320} >= {(0, 0), (30, 0), (30, 640)} and (60, 1280) in {c["gstat"][1:] for c in gs if c["N"] == 640}
    # a seam inside a column tile, at its first and at its last column (cpg = 30 at N = 320, tiles of 160: 150 | 180 straddles column 160,
    # a group starts at column 0 of the first source and ends at column 319 + 640 = 959 of the second)
    assert 160 % 30 and 0 % 30 == 0 and (640 + 320) % 30 == 0
    ta = FR.tattn_cases()
    assert {(c["B"], c["HW"], c["heads"], c["K"]) for c in ta if c["route"] == "tattn"} == set(FR.TATTN_SHAPES)
    assert {c["nparts"] for c in ta} == {0, 1, 2, 3} and {c["causal"] for c in ta} == {False, True} and any(c["bias"] for c in ta)
    assert any(c["regime"] == "peaked" for c in ta) and [c["K"] for c in ta if c["route"] == "refused"] == [72]
    # un-gathered statistics are another row's wherever a tile holds more than one pixel
    idx = FR.tile_row_of(3, 20)
    assert (idx != torch.arange(idx.numel())).float().mean() > 0.9 and sorted(idx.tolist()) == list(range(idx.numel()))


def test_tattn_restatements_agree():
    """Under the fold the GPU file restates the projection on the fp16 operands the kernel reads (W' = fp16(W diag(gamma))).  That is
    Linear(LayerNorm(x)) with the unfolded weights, within TOL16, in the ordinary regime -- ops.fold_layernorm is right -- while in the
    peaked regime the two float64 restatements alone are further apart than TOL16: the rounding of W' moves the logits, and a softmax
    with one dominant key amplifies it.  So the unfolded form cannot be the reference there."""
    seen = set()
    for c in FR.tattn_cases():
        if c["route"] != "tattn" or not c["nparts"]:
            continue
        o = FR.tattn_operands(c)
        d = FR.tattn_errors(FR.tattn_reference(c, o, unfolded=True)["out"], FR.tattn_reference(c, o)["out"], c)
        seen.add(c["regime"])
        if c["regime"] == "peaked":
            assert d > TOL16, f"{FR.case_id(c)}: {d:.2e}"
        else:
            assert d < TOL16, f"{FR.case_id(c)}: {d:.2e}"
    assert seen == {"", "peaked"}


NEW_LEDGER = {
    "moca_gemm_f16": ["test_ln_store_loop", "test_fold_tiled_routes", "test_fold_persistent_routes", "test_two_source_a", "test_wgroup",
                      "test_gstat_virtual_concat", "test_tattn"],
    "moca_gemm_ln_ok": ["test_ln_store_loop"],
    "moca_gemm_lnfold_ok": ["test_fold_tiled_routes", "test_fold_persistent_routes", "test_tattn"],
    "moca_gemm_tattn_ok": ["test_tattn", "test_tattn_refused"],
    "moca_gemm_cat_ok": ["test_two_source_a"],
    "moca_gemm_wgroup_ok": ["test_wgroup", "test_ln_store_loop"],
    "moca_gemm_route": ["test_ln_store_loop", "test_fold_tiled_routes", "test_two_source_a", "test_tattn"],
}
OLD_LEDGER_SIZE = {"moca_gemm_f16": 3, "moca_gemm_ln_ok": 1, "moca_gemm_lnfold_ok": 2, "moca_gemm_tattn_ok": 1, "moca_gemm_cat_ok": 1,
                   "moca_gemm_wgroup_ok": 2, "moca_gemm_route": 1}


def test_ledger():
    import test_gemm_fused_gpu as G
    for sym, fns in NEW_LEDGER.items():
        for fn in fns:
            assert "test_gemm_fused_gpu::" + fn in SR.LEDGER[sym], (sym, fn)
            assert callable(getattr(G, fn))
        assert len(SR.LEDGER[sym]) >= OLD_LEDGER_SIZE[sym] + len(fns), "the earlier entries stay"
