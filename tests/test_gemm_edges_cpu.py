"""CPU: the route table and the references of tests/test_gemm_edges_gpu.py check themselves (tests/gemm_edges_ref.py).

  test_route_table ..................... every (route, M, gather) of the GPU file runs on the kernel it is meant for under the route's
                                         knobs (ops.gemm_route) and gives that kernel's host-query signature (a dispatch rule that
                                         changes moves the case visibly)
  test_persistent_routes ............... the shapes of the persistent kernels run on those kernels, hold the tile counts they ask for,
                                         and leave them with split-K or eight row tiles fewer
  test_queries_follow_the_route ........ over gemm_edges_ref.query_sweep (shapes x gathers x epilogues x side inputs x knob sets): a
                                         flag's query says yes exactly where the launch of the call with that flag is accepted, and
                                         reports the tile of the kernel that launch runs on
  test_wgroup_skips_persistent_kernels . per-row-group weights never run on a kernel that has none
  test_geometry_cases_tell_errors ...... at every geometry case's shape and seed each wrong float64 restatement that applies
                                         (symmetric pad, stride-2 sampling off by one, upsample halved on one axis, no zeroing across a
                                         video boundary, row add off by one row) exceeds TOL16: the shapes are not too small or symmetric
  test_normalise_splits ................ normalise_splits of csrc/gemm.hip restated; the GPU file sizes its workspace from it"""
import pytest
import torch

import gemm_edges_ref as R
from moca_video_amd import lib as L
from moca_video_amd import ops


@pytest.fixture
def tune():
    saved = []

    def set_(knob, value):
        saved.append((knob, L.set_tuning(knob, value)))
    yield set_
    for knob, old in reversed(saved):
        L.set_tuning(knob, old)


def _host_case(kind, M, N, C, geo=None):
    """host tensors and keywords of a call shaped like the GPU file's (the queries read pointers, never memory)"""
    if kind == "linear":
        return torch.empty(M, C, dtype=torch.float16), ops.pack_linear(torch.zeros(N, C), torch.zeros(N), device="cpu"), {}
    x = torch.empty(R.geo_source(geo, C), dtype=torch.float16)
    if kind == "tconv":
        return x, ops.pack_tconv3(torch.zeros(N, C, 3, 1, 1), torch.zeros(N), device="cpu"), dict(mode=L.MOCA_A_TCONV3, tconv=(C, geo["T"], geo["HW"]))
    oh, ow = R.geo_out(geo)
    return x, ops.pack_conv3x3(torch.zeros(N, C, 3, 3), torch.zeros(N), device="cpu"), \
        dict(mode=L.MOCA_A_CONV3X3, conv=(C, geo["H"], geo["W"], oh, ow, geo["stride"], geo["up"], geo["nopad"]))


def _out(n):
    """an output of n columns (gemm_route reads its pointer and row stride)"""
    return torch.empty(1, n, dtype=torch.float16)


@pytest.mark.parametrize("route", list(R.ROUTES))
def test_route_table(route, tune):
    spec = R.ROUTES[route]
    for k, v in spec["knobs"].items():
        tune(k, v)
    for N in R.route_Ns(route):
        for M in spec["M"]:
            for K in R.route_Ks(route):
                a, pw, kw = _host_case("linear", M, N, K)
                got = R.signature(route, a, pw, M=M, force_small=R.needs_force_small(route, M), **kw)
                assert got == R.expected_signature(route), (route, M, N, K, got)
                assert ops.gemm_route(a, pw, _out(N), M=M, force_small=R.needs_force_small(route, M), **kw) == R.ROUTE_ID[route], (route, M, N, K)
    N = spec["N"]
    if spec["conv"]:
        for name, geo in R.GEOS.items():
            for C in (64,) + ((8,) if spec["slow"] else ()):
                M = R.geo_M(geo)
                a, pw, kw = _host_case(geo["kind"], M, N, C, geo)
                got = R.signature(route, a, pw, M=M, force_small=R.needs_force_small(route, M), **kw)
                assert got == R.expected_signature(route, linear=False), (route, name, C, got)
                assert ops.gemm_route(a, pw, _out(N), M=M, force_small=R.needs_force_small(route, M), **kw) == R.ROUTE_ID[route], (route, name, C)
    if route == "ws":                                  # M = 32: refused by the weight-stationary kernel, runs on the 128-row kernel
        a, pw, kw = _host_case("linear", 32, N, spec["K"])
        assert R.signature("small128", a, pw, M=32) == (0, 0, False)
        assert ops.gemm_route(a, pw, _out(N), M=32) == R.ROUTE_ID["small64"]      # (N = 320: 64-column tiles)
    # split-K, fp32 output: no statistics epilogue on any route
    if route in R.SPLIT_ROUTES:
        a, pw, kw = _host_case("linear", spec["M"][-1], N, 192)
        fs = R.needs_force_small(route, spec["M"][-1])
        assert R.signature(route, a, pw, M=spec["M"][-1], splits=2, force_small=fs)[:2] == (0, 0)
        assert R.signature(route, a, pw, M=spec["M"][-1], out_f32=True, force_small=fs)[:2] == (0, 0)


@pytest.mark.parametrize("name", list(R.PERSISTENT))
def test_persistent_routes(name, tune):
    spec = R.PERSISTENT[name]
    for k, v in spec["knobs"].items():
        tune(k, v)
    M, N, K = R.PERSISTENT_SHAPE[name]
    assert R.persistent_tiles(name, M, N) >= spec["min_tiles"] and M % spec["tile"][0] != 0, "enough tiles for the kernel, and an M tail"
    a, pw, kw = _host_case("linear", M, N, K)
    assert ops.gemm_lnfold_ok(a, pw, M=M, lnfold=(None, 1, 1e-5)), "every persistent kernel carries the LayerNorm fold"
    want = R.ROUTE_ID[name]
    a = torch.empty(1, K + 24, dtype=torch.float16)[:, :K]            # (lda = K + 24, as the GPU file embeds A)
    pwg = ops.PackedWeight(pw.w, pw.bias, pw.N, pw.K, pw.N // 2, geglu=True)
    assert ops.gemm_route(a, pw, _out(N), M=M) == want and ops.gemm_route(a, pwg, _out(N // 2), M=M) == want
    # the call leaves the kernel, for another one, with two splits (K = 128: at K = 64 normalise_splits leaves one) or 8 row tiles fewer.
    # (The 256 x 256 staggered kernel is not persistent: it has split-K, and its tile count takes the splits in.)
    a2, pw2, _ = _host_case("linear", M, N, 128)
    assert ops.gemm_route(a2, pw2, _out(N), M=M) == want
    split = ops.gemm_route(a2, pw2, _out(N), M=M, splits=2, splitk_ws=torch.empty(1))
    assert split == want if name == "sq256" else split not in (0, want)
    assert ops.gemm_route(a, pw, _out(N), M=M - 8 * spec["tile"][0]) not in (0, want)
    if name == "sq256":                                # the 256 x 256 staggered kernel has no column sums; the 256-row kernel it replaces has
        assert ops.gemm_colsum_rows(a, pw, M=M) == 0
        tune(R.SQ256, 0)
        assert ops.gemm_colsum_rows(a, pw, M=M) == 256


def test_queries_follow_the_route():
    lib = L.load()
    seen, routes = dict.fromkeys(R.QUERIES, 0), set()

    def visit(knobs, label, p):
        what = (knobs, label)
        for q in R.FLAG_QUERIES:
            ans, route = R.ask(q, p), lib.moca_gemm_route(R.flagged(p, q))
            seen[q] += ans != 0
            routes.add(route)
            if q == "colsum_rows" and (p.flags & L.MOCA_EP_GSTAT) and ans and p.M % ans:
                assert route == 0, (q, what)           # (the sweep's one statistics group of M rows is not whole row tiles)
                continue
            assert (ans != 0) == (route != 0), (q, ans, route, what)
            if q == "colsum_rows":
                assert ans == (R.ROUTE_TILE[route][0] if route else 0), (q, ans, route, what)
            elif q == "rowsum_cols":
                assert ans == (R.ROUTE_TILE[route][1] if route else 0), (q, ans, route, what)
            elif q == "tattn_ok":
                assert route in (0, L.MOCA_ROUTE_TATTN), (q, route, what)
        route = lib.moca_gemm_route(p)
        routes.add(route)
        wg, cat, skgn = R.ask("wgroup_ok", p), R.ask("cat_ok", p), R.ask("splitk_groupnorm_ok", p)
        assert wg == (p.wgroup_rows > 0 and route != 0) and cat == (bool(p.a2) and route != 0), (wg, cat, route, what)
        assert not skgn or lib.moca_gemm_route(R.flagged(p, "splitk_groupnorm_ok")) != 0, what
        for q, v in (("wgroup_ok", wg), ("cat_ok", cat), ("splitk_groupnorm_ok", skgn)):
            seen[q] += v != 0
    R.query_sweep(visit)
    assert all(seen.values()), f"a query never said yes: {seen}"
    assert routes == set(R.ROUTE_TILE) | {0}, f"routes the sweep never reached: {set(R.ROUTE_TILE) - routes}"


@pytest.mark.parametrize("knobs", [{R.SQP: 2, R.G4P: 0, R.WS: 0}, {R.SQP: 0, R.G4P: 2, R.WS: 0}], ids=["sqp", "g4p"])
def test_wgroup_skips_persistent_kernels(knobs, tune):
    """M = 13440 = two groups of 42 x 160 rows, N = 1280, K = 64: 265 / 530 tiles, enough for either persistent kernel -- which would
    run group 1's rows against group 0's weights.  The call runs where gemm_wgroup_ok has always said it does: the 160 x 320 tiling."""
    for k, v in knobs.items():
        tune(k, v)
    M, N, K = 13440, 1280, 64
    a, pw, _ = _host_case("linear", M, N, K)
    name = "sqp" if knobs[R.SQP] else "g4p"
    assert R.persistent_tiles(name, M, N) >= R.PERSISTENT[name]["min_tiles"]
    assert ops.gemm_route(a, pw, _out(N), M=M) == R.ROUTE_ID[name]
    wgroup = (M // 2, N * pw.w.stride(0))
    assert ops.gemm_wgroup_ok(a, pw, M=M, wgroup=wgroup)
    assert ops.gemm_route(a, pw, _out(N), M=M, wgroup=wgroup) == L.MOCA_ROUTE_W80W


@pytest.mark.parametrize("name", list(R.GEOS))
def test_geometry_cases_tell_errors(name):
    geo = R.GEOS[name]
    wrongs = R.wrongs_of(geo)
    assert len(wrongs) >= 2 or name == "s1", "every gather parameter of the case has its wrong restatement"
    for C, N in ((8, 64), (64, 320)):
        right = R.random_geo_case(geo, C, N, R.geo_seed(name))
        assert right["rowadd"].shape[0] >= 2, "more than one row-add group"
        for wrong in wrongs:
            bad = R.random_geo_case(geo, C, N, R.geo_seed(name), wrong=wrong)
            for key in ("x", "w", "rowadd", "res"):
                assert torch.equal(bad[key], right[key])
            worst = R.block_errors(bad["ref"], right["ref"]).max().item()
            assert worst > 10 * R.TOL16, f"{name} C={C} N={N}: the {wrong} restatement is only {worst:.1e} away"
        # the probe sees every tap, and every source pixel through some tap
        x, w, exp = R.probe_case(geo, C, N)
        taps = 3 if geo["kind"] == "tconv" else 9
        live = [bool((exp[:, n] > 0).any()) for n in range(taps)]
        assert exp.max() <= 2048 and (live == [False, True, False] if geo.get("T") == 1 else all(live))     # (T = 1: both neighbours are padding)
        if not (geo["kind"] == "conv" and geo["stride"] == 2):
            assert set(exp.unique().long().tolist()) >= set(range(1, int(x[..., 0].max()) + 1))


def test_phase_probe_matches_restatement():
    for phase in (1, 2, 3, 4):
        x, w, exp = R.phase_probe_case(R.PHASE_GEO, 8, 64, phase)
        assert torch.equal(R.ref_phase(x, w, phase), exp)
    # the four phases of packed 3x3 weights add up to upsample + conv (ops.pack_upconv_phases)
    g = R.gen(5)
    xr, w3 = R.randh(g, 2, 5, 7, 8), R.randh(g, 64, 8, 3, 3, scale=0.1)
    full = R.ref_conv(xr, w3, up=1).view(2, 10, 14, 64)
    for ph, pw in enumerate(ops.pack_upconv_phases(w3.float(), None, device="cpu")):
        a, b = ph >> 1, ph & 1
        got = R.ref_phase(xr, pw.w[:64, :32], ph + 1)
        assert (got - full[:, a::2, b::2]).abs().max() < 2e-3 * full.abs().max()


def test_normalise_splits(tune):
    for (ktiles, splits), want in R.SPLIT_CASES.items():
        assert R.normalise_splits(ktiles * 64, splits) == want, (ktiles, splits)
    assert R.normalise_splits(72, 2) == 2 and R.normalise_splits(64, 8) == 1 and R.normalise_splits(328, 4) == 3
    # the library agrees where a query shows it: a split-K call has no column sums, one that normalises to 1 split does
    for k, v in R.ROUTES["glds128"]["knobs"].items():
        tune(k, v)
    for K, splits in ((64, 8), (128, 2), (320, 4), (192, 1)):
        a, pw, kw = _host_case("linear", 300, 128, K)
        assert (ops.gemm_colsum_rows(a, pw, M=300, splits=splits) == 256) == (R.normalise_splits(K, splits) == 1), (K, splits)
    assert L.load().moca_gemm_splitk_ws_bytes(300, 128, 3) == 3 * 300 * 128 * 4


def test_span_limit():
    M = 4100
    lda = R.lda_at_span_limit(M)
    assert lda % 8 == 0 and R.a_span_bytes_linear(M, lda) >= 1 << 31 > R.a_span_bytes_linear(M, lda - 8)
    assert ((M - 1) * (lda - 8) + 127) * 2 > (1 << 31) - (1 << 20), "the last row's offsets sit within 1 MiB of the top of the 32-bit range"
