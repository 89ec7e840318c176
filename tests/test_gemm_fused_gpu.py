"""GPU: what moca_gemm_f16 does beyond bias, row add, residual and GEGLU (csrc/gemm_device.h store_fp16_tile_ln, lnfold_issue / _finish /
_apply as the tiled kernels and g4p / g4q call them, lnfold_stats under sqp's stat_read in gemm_persistent.hip, the two-source gather and the per-row-group weights of gemm_w80s_kernel.inc / gemm_ws.hip,
MOCA_EP_GSTAT with gstat_cpg / gstat_coff, the MOCA_EP_TATTN epilogue), on the kernel each case is meant for, against float64 torch on
the same fp16 operands (tests/gemm_fused_ref.py: the case tables, checked without a device by tests/test_gemm_fused_cpu.py).

  A  test_ln_store_loop ............ MOCA_EP_LN: both outputs, tails of 1 and 161 rows, ld_ln != ldo, in-place residual, per-group
                                     weights, residual rows offset by 40 / 100, gamma = 0 exact, the row power of a unit-gamma launch
  B  test_fold_tiled_routes ........ MOCA_EP_LNFOLD on glds128, glds160, g4, w80, w80w: synthetic partials (nparts 1, 2, 3, 10), every
     test_fold_persistent_routes     row its own mean and spread, a constant row, a block with |mean| / std = 100; GEGLU on g4; the
                                     same on sq256 / g4p / g4q / sqp at their minimum shapes
  C  test_two_source_a ............. a2 on w80 / w80w: NaN behind both sources' columns, float64 on the concatenation and bit-equality
                                     with the same kernel on the materialised concat; under the persistent kernels' knobs
  D  test_wgroup ................... per-row-group weights on w80 / w80w / ws: NaN between the groups' matrices, per-group bias
  E  test_gstat_virtual_concat ..... MOCA_EP_GSTAT with (cpg, coff) on glds128, glds160, w80, w80w: every accumulator
  F  test_tattn, test_tattn_refused  MOCA_EP_TATTN plain / causal, with the fold; per (video, head) slice and per pixel-within-tile

Every case asserts its route (ops.gemm_route) and its feature's query first.  The error is taken per block of 64 output rows (F: per
slice and per pixel) against TOL16; the large-mean blocks of A and B add twice the error of the same formula in fp32 torch (printed).
Every output buffer -- out, ln_out, row-sum partials, column sums, accumulators -- has canaries behind its last row and in its pad
columns.  No case is skipped."""
import pytest
import torch

import gemm_edges_ref as R
import gemm_fused_ref as FR
from attention_edges_ref import check_slices
from gemm_edges_ref import TOL16

pytestmark = pytest.mark.gpu

from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

DEV = "cuda"
WORST = {}                      # section -> worst ratio of an error to its bound


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for sec, worst in sorted(WORST.items()):
        print(f"[worst] section {sec}: {worst:.3f} of its bound")
    torch.cuda.empty_cache()


@pytest.fixture
def tune():
    """kernel-choice knobs (include/moca_hip.h MOCA_TUNE_*), every one restored afterwards"""
    saved = []

    def set_(knob, value):
        saved.append((knob, L.set_tuning(knob, value)))
    yield set_
    for knob, old in reversed(saved):
        L.set_tuning(knob, old)


def take(tune, c):
    for k, v in FR.case_knobs(c).items():
        tune(k, v)


def note(sec, ratio):
    WORST[sec] = max(WORST.get(sec, 0.0), ratio)


def blocks(got, ref, what, sec, tol=TOL16):
    """every 64-row block within its bound (`tol`: a number or one per block)"""
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    e = R.block_errors(got, ref)
    ratio = (e / tol).max().item()
    note(sec, ratio)
    print(f"[parity] {what}: worst 64-row block {e.max().item():.2e} of its max|ref|, {ratio:.3f} of its bound")
    assert ratio <= 1.0, f"{what}: block errors {[f'{v:.1e}' for v in e.tolist()]}"


def stat(e, tol, what, sec):
    note(sec, e / tol)
    print(f"[stats] {what}: {e:.2e} (bound {tol:.1e})")
    assert e <= tol, f"{what}: off by {e:.2e}"


def check_rowsum(t, what, sec):
    """the partials, summed over the column tiles, are the float64 row sums of the STORED values, per block of 64 rows"""
    c = t["c"]
    M, cols = c["M"], FR.tile_cols(c["route"])
    assert torch.isnan(t["rsbuf"][:512]).all() and torch.isnan(t["rsbuf"][-512:]).all(), f"{what}: row sums written outside [N / cols][M][2]"
    assert torch.isfinite(t["rs"]).all(), f"{what}: a row's partial sums were not written"
    ps = t["rs"].view(c["N"] // cols, M, 2).double().sum(0).cpu()
    of = t["out"].double().cpu()
    for j, ref in enumerate((of.sum(1), (of * of).sum(1))):
        stat(R.block_errors(ps[:, j:j + 1], ref[:, None]).max().item(), FR.TOL_ROWSUM, f"{what} row sums [{j}]", sec)


def check_colsum(t, ref, what, sec):
    c = t["c"]
    M, N, tm = c["M"], c["N"], FR.tile_rows(c["route"])
    tiles = (M + tm - 1) // tm
    assert torch.isnan(t["csbuf"][0]).all() and torch.isnan(t["csbuf"][-1]).all(), f"{what}: column sums written for a tile past ceil(M / rows)"
    got = t["cs"].view(tiles, N, 2).double().cpu()
    assert torch.isfinite(got).all(), f"{what}: a tile's sums were not written"
    rt = torch.nn.functional.pad(ref, (0, 0, 0, tiles * tm - M)).view(tiles, tm, N)
    for j, want in enumerate((rt.sum(1), (rt * rt).sum(1))):
        e = ((got[..., j] - want).abs().amax(-1) / want.abs().amax(-1)).max().item()
        stat(e, FR.TOL_COLSUM, f"{what} column sums [{j}]", sec)


def check_gstat(t, ref, what, sec):
    """every (statistics group, channel group) accumulator against the float64 sums of the reference output; the groups this source
    does not touch exactly zero; the accumulators before and behind untouched"""
    assert (t["gsbuf"][0] == FR.GSTAT_CANARY).all() and (t["gsbuf"][-1] == FR.GSTAT_CANARY).all(), f"{what}: an atomic landed outside the accumulators"
    got = t["gs"].double().cpu() * torch.tensor(FR.GSTAT_SCALE, dtype=torch.float64)
    e, zero = FR.pair_errors(got, FR.gstat_expected(t["c"], ref))
    assert zero, f"{what}: a channel group this source does not touch is not zero"
    stat(e, FR.TOL_GSTAT, f"{what} accumulators", sec)


def run_linear(c):
    """one case of sections A .. E under the knobs in force -> its laid-out tensors after the launch"""
    what = FR.case_id(c)
    o = FR.operands(c)
    ref = FR.reference(c, o)
    t = FR.build(c, o, DEV)
    route = ops.gemm_route(t["a"], t["pw"], t["out"], **t["kw"])
    assert route == FR.ROUTE_ID[c["route"]], f"{what}: runs on route {route}"
    ok = FR.feature_ok(t)
    assert ok and all(ok.values()), f"{what}: {ok}"
    ops.gemm(t["a"], t["pw"], t["out"], **t["kw"])
    sec = c["sec"]
    tol, slack = FR.block_tol(c, o, ref)
    if slack.max() > 0:
        print(f"[slack] {what}: twice the fp32 restatement's block error = {slack.max().item():.2e} (TOL16 {TOL16:.1e})")
    blocks(t["out"], ref["out"], what, sec, tol if c["nparts"] else TOL16)
    R.assert_canary(t["obuf"], c["M"], t["out"].shape[1], what)
    if c["ln"]:
        blocks(t["ln"], ref["ln"], what + " ln_out", sec, tol)
        R.assert_canary(t["lnbuf"], c["M"], c["N"], what + " ln_out")
        if c["ln"] == "gamma0":
            assert torch.equal(t["ln"].cpu(), o["beta"].half().expand(c["M"], -1)), f"{what}: gamma = 0 must give fp16(beta) exactly"
        if c["ln"] == "unit":
            y = ref["out"]
            var = ((y - y.mean(1, keepdim=True)) ** 2).mean(1)
            power = (t["ln"].double().cpu() ** 2).mean(1)
            stat((power - var / (var + FR.EPS)).abs().max().item(), FR.TOL_ROWPOWER, f"{what} row power", sec)
    if c["rowsum"]:
        check_rowsum(t, what, sec)
    if c["colsum"]:
        check_colsum(t, ref["out"], what, sec)
    if c["gstat"]:
        check_gstat(t, ref["out"], what, sec)
    if c["nparts"]:
        assert torch.isnan(t["pbuf"][0]).all() and torch.isnan(t["pbuf"][-1]).all()
    return t


def run_all(cases, tune):
    assert cases
    for c in cases:
        take(tune, c)
        run_linear(c)


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("which", ["M161", "M320", "M321", "M641", "edges"])
def test_ln_store_loop(which, tune):
    """the bias x row add x residual matrix at one M (rowadd_div 1, 7, M; K = 64, 192), or the edge cases: out aliasing residual,
    per-group weights, residual offsets 40 / 100, gamma = 0, unit gamma"""
    plain = lambda c: c["ln"] == "std" and not (c["alias"] or c["groups"] or c["res_offset"])
    cases = [c for c in FR.ln_cases() if (plain(c) and which == f"M{c['M']}") or (not plain(c) and which == "edges")]
    run_all(cases, tune)


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("route", FR.FOLD_ROUTES)
def test_fold_tiled_routes(route, tune):
    run_all([c for c in FR.fold_cases() if c["route"] == route], tune)


@pytest.mark.parametrize("name", list(R.PERSISTENT))
def test_fold_persistent_routes(name, tune):
    """the persistent kernels prefetch the NEXT tile's statistics: every row has its own, so a tile that takes another tile's is wrong"""
    run_all([c for c in FR.fold_cases() if c["route"] == name], tune)


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("route", ["w80", "w80w", "persistent_knobs"])
def test_two_source_a(route, tune):
    cases = [c for c in FR.cat_cases() if (c["under"] is not None) == (route == "persistent_knobs") and (c["under"] or c["route"] == route)]
    assert cases
    for c in cases:
        take(tune, c)
        t = run_linear(c)
        # the same kernel on the materialised concat: same k order, so bit for bit -- the output and every statistic
        flat = dict(c, k1=0)
        o = FR.operands(flat)
        m = FR.build(flat, o, DEV)
        kw = m["kw"]
        if c["under"]:                                 # (without a second source the persistent kernel would take the call: its knob off)
            for k in (R.SQP, R.G4P):
                tune(k, 0)
        assert ops.gemm_route(m["a"], m["pw"], m["out"], **kw) == FR.ROUTE_ID[c["route"]]
        ops.gemm(m["a"], m["pw"], m["out"], **kw)
        what = FR.case_id(c)
        assert torch.equal(t["out"], m["out"]), f"{what}: two-source A differs from the materialised concat"
        for key in ("rs", "cs", "gs"):
            if key in t:
                assert torch.equal(t[key], m[key]), f"{what}: {key} differs from the materialised concat"


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("route", ["w80", "w80w", "ws"])
def test_wgroup(route, tune):
    run_all([c for c in FR.wgroup_cases() if c["route"] == route], tune)


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("route", FR.GSTAT_ROUTES)
def test_gstat_virtual_concat(route, tune):
    run_all([c for c in FR.gstat_cases() if c["route"] == route], tune)


# ---------------------------------------------------------------- F
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("shape", FR.TATTN_SHAPES, ids=lambda s: "B%d_HW%d_h%d_K%d" % s)
def test_tattn(shape, causal, tune):
    cases = [c for c in FR.tattn_cases() if (c["B"], c["HW"], c["heads"], c["K"]) == shape and c["causal"] == causal and c["route"] == "tattn"]
    assert len(cases) == 6
    for c in cases:
        what = FR.case_id(c)
        o = FR.tattn_operands(c)
        ref = FR.tattn_reference(c, o)
        t = FR.tattn_build(c, o, DEV)
        assert ops.gemm_tattn_ok(t["a"], t["pw"], **t["kw"]), what
        assert ops.gemm_route(t["a"], t["pw"], t["out"], **t["kw"]) == L.MOCA_ROUTE_TATTN, what
        ops.gemm(t["a"], t["pw"], t["out"], **t["kw"])
        got = t["out"].cpu()
        note("F", check_slices(got, ref["out"], c["B"], c["heads"], what) / TOL16)
        pe = FR.pixel_errors(got, ref["out"], c)
        note("F", pe.max().item() / TOL16)
        print(f"[parity] {what}: worst pixel-within-tile {pe.max().item():.2e} (pixel {pe.argmax().item()})")
        assert pe.max().item() <= TOL16, f"{what}: pixel errors {[f'{v:.1e}' for v in pe.tolist()]}"
        R.assert_canary(t["obuf"], c["M"], 64 * c["heads"], what)
        if causal:                                     # frame 0 sees itself alone: its rows are the v projection of frame 0
            f0 = lambda x: x.reshape(c["B"], FR.T_FRAMES, c["HW"], -1)[:, 0]
            note("F", check_slices(f0(got), f0(ref["v"]), c["B"], c["heads"], what + " frame 0 = v") / TOL16)
        if c["nparts"]:
            assert torch.isnan(t["pbuf"][0]).all() and torch.isnan(t["pbuf"][-1]).all()


def test_tattn_refused():
    """K = 72 is no whole number of k-tiles: the query says no, and the launch returns the bad-argument code and writes nothing"""
    (c,) = [c for c in FR.tattn_cases() if c["route"] == "refused"]
    t = FR.tattn_build(c, FR.tattn_operands(c), DEV)
    assert not ops.gemm_tattn_ok(t["a"], t["pw"], **t["kw"]) and ops.gemm_route(t["a"], t["pw"], t["out"], **t["kw"]) == 0
    with pytest.raises(L.MocaHipError):
        ops.gemm(t["a"], t["pw"], t["out"], **t["kw"])
    torch.cuda.synchronize()
    assert torch.isnan(t["obuf"]).all(), "refused, but the output was written"
