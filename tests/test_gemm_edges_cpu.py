"""CPU: the route table and the references of tests/test_gemm_edges_gpu.py check themselves (tests/gemm_edges_ref.py).

  test_route_table ..................... every (route, M, gather) of the GPU file gives the host-query signature of the kernel it is
                                         meant for under the route's knobs (a dispatch rule that changes moves the case visibly)
  test_persistent_routes ............... the shapes of the persistent kernels hold the tile counts those kernels ask for
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
    N = spec["N"]
    if spec["conv"]:
        for name, geo in R.GEOS.items():
            for C in (64,) + ((8,) if spec["slow"] else ()):
                M = R.geo_M(geo)
                a, pw, kw = _host_case(geo["kind"], M, N, C, geo)
                got = R.signature(route, a, pw, M=M, force_small=R.needs_force_small(route, M), **kw)
                assert got == R.expected_signature(route, linear=False), (route, name, C, got)
    if route == "ws":                                  # M = 32: refused by the weight-stationary kernel, runs on the 128-row kernel
        a, pw, kw = _host_case("linear", 32, N, spec["K"])
        assert R.signature("small128", a, pw, M=32) == (0, 0, False)
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
    assert R.persistent_ok(name, M, N, K, K + 24) and R.persistent_ok(name, M, N, K, K + 24, geglu=True)
    assert not R.persistent_ok(name, M, N, K, K + 24, splits=2) and not R.persistent_ok(name, M - 8 * spec["tile"][0], N, K, K + 24)
    if name == "sq256":                                # the 256 x 256 staggered kernel has no column sums; the 256-row kernel it replaces has
        assert ops.gemm_colsum_rows(a, pw, M=M) == 0
        tune(R.SQ256, 0)
        assert ops.gemm_colsum_rows(a, pw, M=M) == 256


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
