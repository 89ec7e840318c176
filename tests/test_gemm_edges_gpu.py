"""GPU: moca_gemm_f16 (csrc/gemm.hip, gemm_tiled.hip, gemm_w80s_kernel.inc, gemm_persistent.hip, gemm_ws.hip) on every dispatch route at its gather, stride, tail and epilogue
edges, against float64 torch on the same fp16 operands (tests/gemm_edges_ref.py).  The error is taken per block of 64 output rows --
max|got - ref| over the block / max|ref| of that block -- and every block must meet TOL16 = 3e-3 (fp32 output: 1e-3).  Bias, row add
and residual are drawn at scale 1, so dropping or misplacing one of them is an O(1) error.

Which gap of the kernel-level suite each test closes:
  1. gather geometry on the big kernels (stride 2, up, nopad_lo, T in
     {1, 2, 3, 16}, B = 3, up_phase; zero page / descriptor range check /
     slow_src halos), exact and random ................................ test_index_probe, test_geometry_random_operands
  2. lda > K, ldo > N, ldr > N, ld_rowadd > N, pad columns, guard rows .. test_strides_pad_columns_guard_rows,
     (lda = 2c with fp32 output; GEGLU with ldo = N / 2 + 8;              test_strides_vae_scores_f32, test_strides_geglu,
      the persistent kernels) ..........................................  test_persistent_routes_strides_and_epilogues
     (per-row-group weights under the persistent kernels' knobs) ...... test_wgroup_never_on_persistent_kernels
  3. row add on w80 (both tilings), g4, the 128-row kernel, the split-K
     reduce; rowadd_div straddling row tiles .......................... test_epilogue_matrix
     (the same on sq256 / g4p / g4q / sqp) ............................ test_persistent_routes_strides_and_epilogues
  4. fp32 output with split-K, BN 64 / 128 / 160, M <= 128 ............. test_f32_output, test_strides_vae_scores_f32
     (GELU at M = 128 / 129, GEGLU through the reduce) ................ test_gelu_tile_edge, test_geglu_splitk
  5. normalise_splits lowering the factor; MOCA_TUNE_SLAB_F16;
     MOCA_TUNE_SQP_WALK ............................................... test_splitk_normalisation, test_splitk_fp16_slabs, test_sqp_walk
  6. prefetch blocks appended to the grid ............................. test_prefetch_blocks_change_nothing
  7. streaming-store instantiations (output >= 128 MiB) ............... test_streaming_stores, test_streaming_stores_persistent
  8. buffer_addressable: the fall-through at 2^31 bytes and the top of
     the 32-bit offset range .......................................... test_address_range
  9. column / row statistics at an M tail ............................. test_statistics_at_m_tail
 (I) every statistics / fold flag: query 0 <-> launch refused ......... test_query_and_launch_agree

Every case asserts, through ops.gemm_route and the host queries, that it runs on the kernel it is meant for (gemm_edges_ref.ROUTES /
PERSISTENT, checked without a device by tests/test_gemm_edges_cpu.py).
B, C, D, G and I run every route at two column counts (gemm_edges_ref.ROUTES: N and N2, up to six column tiles)."""
import functools

import pytest
import torch

import gemm_edges_ref as R
from gemm_edges_ref import NAN, TOL16, TOL32, assert_route, geo_kw, launch, pack

pytestmark = pytest.mark.gpu

from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, worst in sorted(R.WORST.items()):
        print(f"[worst] group {group}: {worst:.2e} (TOL16 {TOL16:.1e}, fp32 {TOL32:.1e})")
    for cache in (geo_case, lin_case, big_operands):   # (host cases and ~300 MB of device operands: not kept for the rest of the session)
        cache.cache_clear()
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


def take(tune, route):
    for k, v in (R.ROUTES.get(route) or R.PERSISTENT[route])["knobs"].items():
        tune(k, v)


def gather_paths(route):
    return ("fast", "slow") if R.ROUTES[route]["slow"] else ("fast",)


ROUTE_GATHER = [(r, g) for r in R.CONV_ROUTES for g in gather_paths(r)]


def check(out, obuf, case, what, group, tol=TOL16):
    worst = R.check_blocks(out, case["ref"], what, tol=tol, group=group)
    if obuf is not None:
        R.assert_canary(obuf, out.shape[0], out.shape[1], what)
    return worst


@functools.lru_cache(maxsize=32)
def geo_case(name, C, N):
    return R.random_geo_case(R.GEOS[name], C, N, R.geo_seed(name))


@functools.lru_cache(maxsize=8)
def lin_case(seed, M, N, K, bias=True, div=0, res=False, act=None):
    return R.linear_case(seed, M, N, K, bias, div, res, act)


# ---------------------------------------------------------------- A. gather geometry
def phase_routes(route, gather):
    return route in R.BIG_ROUTES and gather == "fast"      # (the entry accepts up_phase with M > 160, fast gather, 256- / 320-row kernels)


@pytest.mark.parametrize("route,gather", ROUTE_GATHER)
def test_index_probe(route, gather, tune):
    """Source pixel i carries the code 1 + i in channel 0; column n of W has a single 1.0 at tap n % 9 (n % 3): the output must be the
    shifted, zero-padded code image BIT FOR BIT.  3x3 stride 1; stride 2 on 9 x 11 and 10 x 12; stride 2 with nopad_lo (even grid);
    up; temporal conv with T in {1, 2, 3, 16}, B = 3; up_phase 1..4.  M = 321 .. 396: two row tiles with a tail on every kernel; halo
    rows through the zero page (glds / g4 fast), the descriptor range check (w80) and slow_src (C = 8)."""
    take(tune, route)
    C, N = (64 if gather == "fast" else 8), R.ROUTES[route]["N"]
    for name, geo in R.GEOS.items():
        x, w, exp = R.probe_case(geo, C, N)
        case = dict(x=x, w=w, bias=None, M=R.geo_M(geo))
        out, obuf, _ = launch(route, case, geo=geo, C=C)
        assert torch.equal(out.double().cpu(), exp), f"probe {route} {gather} {name}: {(out.double().cpu() != exp).sum().item()} wrong codes"
        R.assert_canary(obuf, case["M"], N, f"probe {route} {name}")
    if phase_routes(route, gather):
        geo = R.PHASE_GEO
        Fr, H, W = geo["Fr"], geo["H"], geo["W"]
        for phase in (1, 2, 3, 4):
            a_, b_ = (phase - 1) >> 1, (phase - 1) & 1
            x, w2d, exp = R.phase_probe_case(geo, C, N, phase)
            out = torch.full((Fr, 2 * H, 2 * W, N), NAN, dtype=torch.float16, device=DEV)
            pw = ops.pack_linear(w2d, None)
            a = x.to(DEV).reshape(-1, C)
            kw = geo_kw(geo, C, up_phase=phase)
            assert_route(route, a, pw, Fr * H * W, dict(kw, up_phase=phase))
            ops.gemm(a, pw, out.view(-1, N), M=Fr * H * W, up_phase=phase, **kw)
            assert torch.equal(out[:, a_::2, b_::2].double().cpu(), exp), f"probe {route} up_phase {phase}"
            written = torch.zeros(2 * H, 2 * W, dtype=torch.bool, device=DEV)
            written[a_::2, b_::2] = True
            assert torch.isnan(out[:, ~written]).all(), f"probe {route} up_phase {phase}: wrote a pixel of another phase"


@pytest.mark.parametrize("route,gather", ROUTE_GATHER)
def test_geometry_random_operands(route, gather, tune):
    """the same geometry list with random operands, bias, a per-frame row add and a residual (all scale 1), against float64"""
    take(tune, route)
    C, N = (64 if gather == "fast" else 8), R.ROUTES[route]["N"]
    for name, geo in R.GEOS.items():
        case = geo_case(name, C, N)
        out, obuf, _ = launch(route, case, geo=geo, C=C)
        check(out, obuf, case, f"geometry {route} {gather} {name} M={case['M']}", "A")
    if phase_routes(route, gather):
        geo = R.PHASE_GEO
        Fr, H, W = geo["Fr"], geo["H"], geo["W"]
        g = R.gen(7900)
        x = R.randh(g, Fr, H, W, C)
        w3, bias = R.randh(g, N, C, 3, 3, scale=(9 * C) ** -0.5), torch.randn(N, generator=g)
        out = torch.full((Fr, 2 * H, 2 * W, N), NAN, dtype=torch.float16, device=DEV)
        ref = torch.zeros(Fr, 2 * H, 2 * W, N, dtype=torch.float64)
        for ph, pw in enumerate(ops.pack_upconv_phases(w3.float(), bias)):
            ops.gemm(x.to(DEV).reshape(-1, C), pw, out.view(-1, N), M=Fr * H * W, up_phase=ph + 1, **geo_kw(geo, C, up_phase=ph + 1))
            ref[:, ph >> 1::2, ph & 1::2] = R.ref_phase(x, pw.w[:N, :4 * C].cpu(), ph + 1) + bias.double()
        R.check_blocks(out.view(-1, N), ref.view(-1, N), f"geometry {route} up_phase 1..4", group="A")


# ---------------------------------------------------------------- B. strides, pad columns, guard rows
@pytest.mark.parametrize("route", list(R.ROUTES))
def test_strides_pad_columns_guard_rows(route, tune):
    """Every operand inside a larger NaN-filled allocation: a [M + 2][K + 24] from row 1, out / residual / row add with ld = N + 8 and a
    guard row above and below.  The result is finite and correct (no read past K or M reaches an MFMA), pad columns and guard rows of
    `out` are still NaN (no stray store).  K = 8 / 72 / 328 (slow gather): the columns behind K of every A row are NaN.  Also `out`
    aliasing `residual`.  Every route at both of its column counts."""
    take(tune, route)
    spec = R.ROUTES[route]
    for N in R.route_Ns(route):
        for M in spec["M"]:
            for K in R.route_Ks(route):                # (K = 8: one k-tile with 8 live columns, lda = 32 < the k-tile)
                div = 0 if route == "ws" else 7       # (the weight-stationary kernel has no row add)
                case = lin_case(100 + M + K, M, N, K, True, div, True)
                for alias in (False, True):
                    out, obuf, _ = launch(route, case, alias=alias)
                    check(out, obuf, case, f"strides {route} M={M} N={N} K={K} alias={alias}", "B")
    N = spec["N"]
    if route == "ws":                                  # M = 32: refused by the weight-stationary kernel (M >= 8192), runs on the 128-row kernel
        case = lin_case(132, 32, N, 320, True, 0, True)
        out, obuf, _ = launch("small64", case, check_route=False)
        check(out, obuf, case, "strides ws knobs M=32 (fall-through)", "B")


@pytest.mark.parametrize("route", ["small64", "small128", "glds128", "glds160"])
def test_strides_vae_scores_f32(route, tune):
    """the VAE attention scores: a = qk[:, :c] with lda = 2c (the k half is NaN here), fp32 output with pad columns and guard rows"""
    take(tune, route)
    N = R.ROUTES[route]["N"]
    for M in R.ROUTES[route]["M"]:
        case = lin_case(150 + M, M, N, 64, False, 0, False)
        out, obuf, _ = launch(route, case, lda_pad=64, out_f32=True)
        check(out, obuf, case, f"strides {route} lda=2c fp32 M={M}", "B", tol=TOL32)


@pytest.mark.parametrize("route", ["g4", "glds128"])
def test_strides_geglu(route, tune):
    """GEGLU: `out` has N / 2 columns (ldo = N / 2 + 8 >= N / 2), strided A"""
    take(tune, route)
    tune(R.G4P, 0), tune(R.SQP, 0)
    for M in R.ROUTES[route]["M"]:
        case = lin_case(170 + M, M, 256, 64, True, 0, False, "geglu")
        out, obuf, _ = launch(route, case, act="geglu")
        check(out, obuf, case, f"strides {route} geglu M={M}", "B")


# ---------------------------------------------------------------- C. epilogue matrix
def combos(route):
    if route in ("w80", "w80w"):
        return [(b, ra, rs) for b in (1, 0) for ra in (1, 0) for rs in (1, 0)]
    if route == "ws":
        return [(1, 0, 1), (0, 0, 0), (0, 0, 1), (1, 0, 0)]
    return [(1, 1, 1), (0, 1, 0), (0, 0, 1)]


@pytest.mark.parametrize("route", list(R.ROUTES))
def test_epilogue_matrix(route, tune):
    """bias x row add x residual (all eight on the w80 routes) with rowadd_div in {1, 7, 100, M} -- groups that straddle row tiles -- at
    every M of the route; then through the split-K reduce (K = 192, splits = 2)"""
    take(tune, route)
    spec = R.ROUTES[route]
    K = spec.get("K", 64)
    for N in R.route_Ns(route):
        for M in spec["M"]:
            for bias, ra, rs in combos(route):
                for div in ((1, 7, 100, M) if ra else (0,)):
                    case = lin_case(200 + M, M, N, K, bool(bias), div, bool(rs))
                    out, obuf, _ = launch(route, case)
                    check(out, obuf, case, f"epilogue {route} M={M} N={N} bias={bias} rowadd={ra}/{div} res={rs}", "C")
    N = spec["N"]
    if route == "ws":                                  # a row add leaves the weight-stationary kernel (moca_gemm_ws_ok)
        M = spec["M"][0]
        case = lin_case(200 + M, M, N, K, True, 7, True)
        pw = pack(case)
        a, ra = case["a"].to(DEV), case["rowadd"].to(DEV)
        assert ops.gemm_rowsum_cols(a, pw, M=M, rowsum=True) == 80 and ops.gemm_rowsum_cols(a, pw, M=M, rowadd=ra, rowadd_div=7, rowsum=True) != 80
        out, obuf, _ = launch(route, case, check_route=False)
        check(out, obuf, case, "epilogue: row add on the 320 -> 320 linear (tiled kernel)", "C")
    if route in R.SPLIT_ROUTES + ("small64",):
        for N in R.route_Ns(route):
            for M in spec["M"][-2:]:
                for div in (1, 7, 100, M):
                    case = lin_case(260 + M, M, N, 192, True, div, True)
                    out, obuf, _ = launch(route, case, splits=2)
                    check(out, obuf, case, f"epilogue {route} split-K reduce M={M} N={N} rowadd/{div}", "C")


@pytest.mark.parametrize("route,N,Ms", [("small64", 64, (1, 77, 300)), ("small128", 128, (1, 77, 300)), ("small64", 320, (1, 77, 300)),
                                        ("small128", 640, (77,)), ("glds128", 128, (300,)), ("glds160", 320, (300,)), ("glds128", 640, (300,))])
@pytest.mark.parametrize("splits", [1, 3])
def test_f32_output(route, N, Ms, splits, tune):
    """fp32 output on the 128-row kernel (M = 1, 77 and, forced, 300; BN = 128 where N % 128 == 0, else BN = 64: N = 64 and the five
    column tiles of N = 320) and on the 256-row kernel (M = 300: BN = 128 at N = 128 / 640, BN = 160 at N = 320); one split and three
    (K = 192: one k-tile per split); bias + row add + residual.  M <= 128 runs on the 128-row kernel under any knobs, so the 256-row
    routes have no such case of their own."""
    take(tune, route)
    assert (N % 128 == 0) == (route in ("small128", "glds128"))        # (moca_gemm_f16: `wide` / big_bn select BN from N alone)
    for M in Ms:
        case = lin_case(300 + M + N, M, N, 192, True, 7, True)
        out, obuf, _ = launch(route, case, splits=splits, out_f32=True)
        check(out, obuf, case, f"fp32 out {route} M={M} N={N} splits={splits}", "C", tol=TOL32)


@pytest.mark.parametrize("N", [64, 128])
def test_gelu_tile_edge(N):
    """MOCA_EP_GELU at M = 128 (one full tile) and 129 (the flag forces the 128-row kernel: a second tile with one row)"""
    for M in (128, 129):
        for K in (64, 72):
            case = lin_case(400 + M + K, M, N, K, True, 0, False, "gelu")
            out, obuf, _ = launch("small64" if N == 64 else "small128", case, act="gelu", check_route=False)
            check(out, obuf, case, f"gelu M={M} N={N} K={K}", "C")


@pytest.mark.parametrize("route", ["g4", "glds128"])
def test_geglu_splitk(route, tune):
    take(tune, route)
    tune(R.G4P, 0), tune(R.SQP, 0)
    for M in (257, 513):
        case = lin_case(450 + M, M, 256, 192, True, 0, False, "geglu")
        out, obuf, _ = launch(route, case, act="geglu", splits=2)
        check(out, obuf, case, f"geglu split-K {route} M={M}", "C")


@pytest.mark.parametrize("route", list(R.PERSISTENT))
def test_persistent_routes_strides_and_epilogues(route, tune):
    """sq256 / g4p / g4q / sqp at their smallest tile counts with an M tail, K = 64: strided A, pad columns and guard rows, bias x row add x
    residual with rowadd_div in {1, 7, 100, M}, `out` aliasing `residual`, and GEGLU (ldo = N / 2 + 8)"""
    take(tune, route)
    M, N, K = R.PERSISTENT_SHAPE[route]
    for bias, ra, rs in combos("g4p"):
        for div in ((1, 7, 100, M) if ra else (0,)):
            case = lin_case(480, M, N, K, bool(bias), div, bool(rs))
            out, obuf, _ = launch(route, case, alias=bool(rs and not ra))
            check(out, obuf, case, f"persistent {route} bias={bias} rowadd={ra}/{div} res={rs}", "C")
    case = lin_case(481, M, N, K, True, 0, False, "geglu")
    out, obuf, _ = launch(route, case, act="geglu")
    check(out, obuf, case, f"persistent {route} geglu", "C")


@pytest.mark.parametrize("name", ["sqp", "g4p"])
def test_wgroup_never_on_persistent_kernels(name, tune):
    """Per-row-group weights under the knobs that send every linear they can run to a persistent kernel: M = 13440 = two groups of
    6720 = 42 x 160 rows, N = 1280, K = 64 -- the smallest shape both persistent kernels accept (265 / 530 tiles against 256 / 512).
    Neither kernel reads wgroup_rows, so the call stays on the 160 x 320 tiling, where gemm_wgroup_ok says it runs; on a persistent
    kernel group 1's rows would meet group 0's weights (an O(1) error).  Each group against float64 of its own weights and bias."""
    take(tune, name)
    M, N, K = 13440, 1280, 64
    rows = M // 2
    g = R.gen(490)
    a = R.randh(g, M, K)
    w = [R.randh(g, N, K, scale=K ** -0.5) for _ in range(2)]
    b = [torch.randn(N, generator=g) for _ in range(2)]
    pws = [ops.pack_linear(w[i], b[i]) for i in range(2)]
    pw = ops.PackedWeight(torch.cat([p.w for p in pws]), torch.cat([p.bias for p in pws]), N, K, N)
    wgroup = (rows, N * pw.w.stride(0))
    ad = a.to(DEV)
    obuf, out = R.canary_out(M, N, DEV)
    assert ops.gemm_route(ad, pws[0], out, M=M) == R.ROUTE_ID[name], "without the groups the persistent kernel takes the call"
    assert ops.gemm_wgroup_ok(ad, pw, M=M, wgroup=wgroup)
    assert ops.gemm_route(ad, pw, out, M=M, wgroup=wgroup) == L.MOCA_ROUTE_W80W
    ops.gemm(ad, pw, out, M=M, wgroup=wgroup)
    for i in range(2):
        ref = R.epilogue(R.ref_linear(a[i * rows:(i + 1) * rows], w[i]), b[i])
        R.check_blocks(out[i * rows:(i + 1) * rows], ref, f"wgroup under the {name} knobs, group {i}", group="C")
    R.assert_canary(obuf, M, N, f"wgroup under the {name} knobs")


# ---------------------------------------------------------------- D. split-K
@pytest.mark.parametrize("route", ["small64"] + list(R.SPLIT_ROUTES))
def test_splitk_normalisation(route, tune):
    """(k-tiles, requested splits) = (5, 4) -> 3, (3, 8) -> 3, (2, 2), (7, 3): the workspace holds exactly the normalised number of slabs
    (NaN beyond it must survive); the result meets TOL16 and is bit-equal across two runs"""
    take(tune, route)
    spec = R.ROUTES[route]
    for (ktiles, splits), norm in R.SPLIT_CASES.items():
        assert R.normalise_splits(ktiles * 64, splits) == norm
        for M, N in [(M, spec["N"]) for M in spec["M"][-2:]] + [(spec["M"][-1], spec["N2"])]:
            case = lin_case(500 + M + ktiles, M, N, ktiles * 64, True, 100, True)
            out, obuf, _ = launch(route, case, splits=splits)
            check(out, obuf, case, f"split-K {route} M={M} N={N} k-tiles={ktiles} splits={splits}->{norm}", "D")
            assert torch.isfinite(launch.ws[:norm * M * N]).all(), "fp32 slabs: every float of the normalised factor's slabs is written"
            out2, _, _ = launch(route, case, splits=splits)
            assert torch.equal(out, out2), f"split-K {route}: two runs differ"


@pytest.mark.parametrize("route", ["glds128", "glds160"])
def test_splitk_fp16_slabs(route, tune):
    """MOCA_TUNE_SLAB_F16 = 1: fp16 partial slabs on the 256-row kernel, still within the fp16 tolerance.  That the knob took effect shows in
    the workspace (sized for fp32 slabs, NaN before the launch): the fp16 slabs [splits][M][N] fill its first half, the second half is
    still NaN (test_splitk_normalisation asserts the opposite without the knob)."""
    take(tune, route)
    tune(L.MOCA_TUNE_SLAB_F16, 1)
    spec = R.ROUTES[route]
    for (ktiles, splits), norm in R.SPLIT_CASES.items():
        for N in R.route_Ns(route):
            M = spec["M"][-1]
            case = lin_case(500 + M + ktiles, M, N, ktiles * 64, True, 100, True)
            out, obuf, _ = launch(route, case, splits=splits)
            check(out, obuf, case, f"fp16 slabs {route} N={N} k-tiles={ktiles} splits={splits}", "D")
            n = norm * M * N
            assert torch.isfinite(launch.ws[:n // 2].view(torch.float16)).all() and torch.isnan(launch.ws[n // 2:n]).all(), "fp16 slabs"


def test_sqp_walk(tune):
    """MOCA_TUNE_SQP_WALK 0 / 1 run the same tiles in another order: both correct, equal to each other (M tail: 8200 = 32 tiles + 8 rows)"""
    take(tune, "sqp")
    M, N, K = R.PERSISTENT_SHAPE["sqp"]
    case = lin_case(600, M, N, K, True, 100, True)
    outs = []
    for walk in (0, 1):
        tune(L.MOCA_TUNE_SQP_WALK, walk)
        out, obuf, _ = launch("sqp", case)
        check(out, obuf, case, f"sqp walk={walk}", "D")
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------- E. prefetch blocks
@pytest.mark.parametrize("route", list(R.BIG_ROUTES) + ["sq256", "g4p", "sqp"])
def test_prefetch_blocks_change_nothing(route, tune):
    """a `prefetch` buffer (1 KiB, 24 KiB + 1 KiB, 3 MiB) appends 24 / 48 blocks to the grid: `out` is bit-equal to the launch without
    one, the buffer is unchanged, the guard rows are intact"""
    take(tune, route)
    if route in R.PERSISTENT:
        M, N, K = R.PERSISTENT_SHAPE[route]
    else:
        M, N, K = R.ROUTES[route]["M"][-1], R.ROUTES[route]["N"], 64
    case = lin_case(700, M, N, K, True, 100, True)
    base, obuf, _ = launch(route, case)
    check(base, obuf, case, f"prefetch {route}: no buffer", "E")
    g = R.gen(701)
    for kib in (1, 25, 3072):
        pf = torch.randint(0, 256, (kib << 10,), dtype=torch.uint8, generator=g).to(DEV)
        assert pf.data_ptr() % 16 == 0
        keep = pf.clone()
        out, obuf, _ = launch(route, case, prefetch=pf)
        assert torch.equal(out, base), f"prefetch {route} {kib} KiB: the output changed"
        assert torch.equal(pf, keep), f"prefetch {route} {kib} KiB: the buffer changed"
        R.assert_canary(obuf, M, N, f"prefetch {route} {kib} KiB")


# ---------------------------------------------------------------- F. streaming stores
STREAM_BYTES = 128 << 20


@functools.lru_cache(maxsize=2)
def big_operands(M, N, K, seed, with_res=True):
    """a [M][K], residual [M][N] on the device (seeded CPU generator), w [N][K], bias"""
    g = R.gen(seed)
    a, w, b = R.randh(g, M, K), R.randh(g, N, K, scale=K ** -0.5), torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g, dtype=torch.float32).half().to(DEV) if with_res else None
    return a.to(DEV), w, b, res


def scan_big(out, a, w, b, res, act=None, tile_rows=0, chunk=10240):
    """float64 reference on the device in row chunks (10240 = a multiple of 64, 160, 256 and 320).  Returns (worst 64-row block error,
    float64 [tiles][N][2] column sums / sums of squares of the reference per `tile_rows` rows or None)."""
    M = out.shape[0]
    wd, bd = w.to(DEV).double(), b.to(DEV).double()
    worst, sums = 0.0, []
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        y = a[r0:r1].double() @ wd.T + bd
        if res is not None:
            y = y + res[r0:r1].double()
        if act == "geglu":
            y = y[:, :y.shape[1] // 2] * R.gelu64(y[:, y.shape[1] // 2:])
        pad = (-(r1 - r0)) % 64
        d = torch.nn.functional.pad((out[r0:r1].double() - y).abs().amax(1), (0, pad)).view(-1, 64).amax(1)
        m = torch.nn.functional.pad(y.abs().amax(1), (0, pad)).view(-1, 64).amax(1)
        worst = max(worst, (d / m.clamp_min(1e-30)).max().item())
        if tile_rows:
            padt = (-(r1 - r0)) % tile_rows
            yt = torch.nn.functional.pad(y, (0, 0, 0, padt)).view(-1, tile_rows, y.shape[1])
            sums.append(torch.stack([yt.sum(1), (yt * yt).sum(1)], -1))
    return worst, (torch.cat(sums) if tile_rows else None)


def stats_close(got, ref, tol, what):
    """per tile: max|got - ref| over the tile's sums / the tile's largest |sum|"""
    assert torch.isfinite(got).all(), f"{what}: a tile's sums were not written"
    for j, name in enumerate(("sums", "sums of squares")):
        e = ((got[..., j].double() - ref[..., j]).abs().amax(-1) / ref[..., j].abs().amax(-1)).max().item()
        print(f"[stats] {what} {name}: {e:.2e} (bound {tol:.1e})")
        assert e <= tol, f"{what}: {name} off by {e:.2e}"


def rowsum_close(part, out, cols, what):
    """the partials, summed, are the float64 row sums of the STORED values within 1e-4"""
    M, N = out.shape
    ps = part.view(N // cols, M, 2).double().sum(0)
    of = out.double()
    for j, ref in enumerate((of.sum(1), (of * of).sum(1))):
        e = ((ps[:, j] - ref).abs().max() / ref.abs().max()).item()
        print(f"[stats] {what} row sums [{j}]: {e:.2e} (bound 1.0e-04)")
        assert e <= 1e-4, f"{what}: row sums [{j}] off by {e:.2e}"


STREAM_CASES = [("w80", 52480, 1280, 64), ("glds128", 52480, 1280, 64), ("g4", 52480, 1280, 64), ("w80w", 209920, 320, 64),
                ("ws", 209920, 320, 320), ("g4-geglu", 52480, 2560, 64)]


@pytest.mark.parametrize("route,M,N,K", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_streaming_stores(route, M, N, K, tune):
    """Output >= 128 MiB: bit 0 of reserved4_ selects the non-temporal instantiation of every store loop (plain, residual, ROWSUM, COLSUM /
    GSTAT; GEGLU: the bit is set from N / 2).  Each against float64 (in row chunks, on the device); the same operands truncated to just
    below the threshold run the other instantiation and must agree bit for bit on the common rows."""
    act = "geglu" if route.endswith("geglu") else None
    route = route.split("-")[0]
    take(tune, route)
    tune(R.G4P, 0), tune(R.SQP, 0), tune(R.SQ256, 0)
    n_out = N // 2 if act else N
    Mlo = (STREAM_BYTES - 1) // (n_out * 2) // 32 * 32      # the largest M % 32 == 0 below the threshold
    assert M * n_out * 2 >= STREAM_BYTES > Mlo * n_out * 2
    a, w, b, res = big_operands(M, N, K, 800 + N, act is None)
    pw = ops.pack_geglu(w, b) if act else ops.pack_linear(w, b)
    assert_route(route, a, pw, M, {})
    cs_rows, rs_cols, _ = R.ROUTES[route]["sig"]
    variants = ["plain"] if act else ["plain", "res"] + (["rowsum"] if rs_cols else []) + (["colsum"] if cs_rows and route != "ws" else []) + \
        (["gstat"] if route == "ws" else [])
    for v in variants:
        obuf, out = R.canary_out(M, n_out, DEV)
        r = res if v != "plain" else None
        kw = {}
        if v == "rowsum":
            kw["rowsum"] = part = torch.full((N // rs_cols * M + 512, 2), NAN, dtype=torch.float32, device=DEV)[:N // rs_cols * M]
        if v == "colsum":
            kw["colsum"] = cs = torch.full(((M + cs_rows - 1) // cs_rows, N, 2), NAN, dtype=torch.float32, device=DEV)
        if v == "gstat":
            gst = torch.zeros(M // cs_rows * 64, dtype=torch.int64, device=DEV)
            kw["gstat"] = (gst, cs_rows)
        ops.gemm(a, pw, out, M=M, residual=r, **kw)
        worst, sums = scan_big(out, a, w, b, r, act, tile_rows=cs_rows if v in ("colsum", "gstat") else 0)
        print(f"[parity] streaming {route} {v} {M}x{N}: worst 64-row block {worst:.2e}")
        R.WORST["F"] = max(R.WORST.get("F", 0.0), worst)
        assert torch.isfinite(out).all() and worst <= TOL16, f"streaming {route} {v}: {worst:.2e}"
        R.assert_canary(obuf, M, n_out, f"streaming {route} {v}")
        if v == "rowsum":
            rowsum_close(part, out, rs_cols, f"streaming {route}")
        if v == "colsum":
            stats_close(cs, sums, 2e-3, f"streaming {route} colsum")
        if v == "gstat":                               # finished statistics: i64 fixed point per (32-row strip, 10-column group)
            gs = gst.view(M // cs_rows, 32, 2).double() * torch.tensor([2.0 ** -20, 2.0 ** -12], dtype=torch.float64, device=DEV)
            x = out.double().view(M // cs_rows, cs_rows, 32, N // 32)
            for j, ref in enumerate((x.sum((1, 3)), (x * x).sum((1, 3)))):
                e = ((gs[..., j] - ref).abs().max() / ref.abs().max()).item()
                assert e <= 1e-3, f"streaming ws gstat [{j}] off by {e:.2e}"
        if v in ("plain", "res"):
            lo = torch.full((Mlo, n_out), NAN, dtype=torch.float16, device=DEV)
            ops.gemm(a[:Mlo], pw, lo, M=Mlo, residual=r[:Mlo] if r is not None else None)
            assert torch.equal(lo, out[:Mlo]), f"streaming {route} {v}: the two store instantiations disagree"
        del obuf, out


@pytest.mark.parametrize("route", ["g4p", "sqp"])
def test_streaming_stores_persistent(route, tune):
    take(tune, route)
    M, N, K = 52480, 1280, 64
    Mlo = (STREAM_BYTES - 1) // (N * 2) // 32 * 32
    assert M * N * 2 >= STREAM_BYTES > Mlo * N * 2 and R.persistent_tiles(route, Mlo, N) >= R.PERSISTENT[route]["min_tiles"]
    a, w, b, res = big_operands(M, N, K, 800 + N)
    pw = ops.pack_linear(w, b)
    assert_route(route, a, pw, M, {}, residual=True)
    for r in (None, res):
        obuf, out = R.canary_out(M, N, DEV)
        ops.gemm(a, pw, out, M=M, residual=r)
        worst, _ = scan_big(out, a, w, b, r)
        print(f"[parity] streaming {route} res={r is not None}: worst 64-row block {worst:.2e}")
        R.WORST["F"] = max(R.WORST.get("F", 0.0), worst)
        assert torch.isfinite(out).all() and worst <= TOL16
        R.assert_canary(obuf, M, N, f"streaming {route}")
        lo = torch.full((Mlo, N), NAN, dtype=torch.float16, device=DEV)
        ops.gemm(a[:Mlo], pw, lo, M=Mlo, residual=r[:Mlo] if r is not None else None)
        assert torch.equal(lo, out[:Mlo]), f"streaming {route}: the two store instantiations disagree"
        del obuf, out


# ---------------------------------------------------------------- G. statistics at an M tail
@pytest.mark.parametrize("route", ["w80", "w80w", "glds128", "glds160"])
def test_statistics_at_m_tail(route, tune):
    """COLSUM at M = rows + 37 and 2 rows + 1 (ceil(M / rows) tiles, as the header documents): every tile's sums -- NaN before the launch --
    equal the float64 column sums of the reference tile within 2e-3 of the tile's largest sum; the rows past M contribute nothing.
    ROWSUM at the same M: the partials, summed, equal the row sums of the stored values within 1e-4."""
    take(tune, route)
    rows, cols, _ = R.ROUTES[route]["sig"]
    for M, N in [(M, N) for N in R.route_Ns(route) for M in (rows + 37, 2 * rows + 1)]:
        case = lin_case(900 + M, M, N, 64, True, 0, True)
        tiles = (M + rows - 1) // rows
        cs_buf = torch.full((tiles + 1, N, 2), NAN, dtype=torch.float32, device=DEV)      # (one spare tile: must stay NaN)
        cs = cs_buf[:tiles]
        out, obuf, pw = launch(route, case, colsum=cs)
        assert torch.isnan(cs_buf[tiles:]).all(), "column sums written for a tile past ceil(M / rows)"
        check(out, obuf, case, f"colsum {route} M={M}", "G")
        a = case["a"].to(DEV)
        assert ops.gemm_colsum_rows(a, pw, M=M, residual=out) == rows
        rt = torch.nn.functional.pad(case["ref"], (0, 0, 0, tiles * rows - M)).view(tiles, rows, N)
        stats_close(cs.cpu(), torch.stack([rt.sum(1), (rt * rt).sum(1)], -1), 2e-3, f"colsum {route} M={M}")
        part_buf = torch.full((N // cols * M + 512, 2), NAN, dtype=torch.float32, device=DEV)      # (512 spare rows: must stay NaN)
        part = part_buf[:N // cols * M]
        out, obuf, _ = launch(route, case, rowsum=part)
        check(out, obuf, case, f"rowsum {route} M={M}", "G")
        assert torch.isnan(part_buf[N // cols * M:]).all(), "row sums written for a row past M"
        assert torch.isfinite(part).all(), "a row's partial sums were not written"
        rowsum_close(part, out, cols, f"rowsum {route} M={M}")


# ---------------------------------------------------------------- H. address range
@pytest.mark.parametrize("where", ["at_limit", "below_limit"])
def test_address_range(where, tune):
    """A linear (M = 4100, K = 128, N = 320) whose A is a strided view of one ~2 GiB allocation, only the K columns written.
    at_limit: a_span_bytes just >= 2^31 leaves the buffer-addressed kernels (the query reports the 256-row kernel), result correct.
    below_limit: the next smaller lda keeps them, the last rows' 32-bit offsets sit at the top of the range: correct on w80 (both
    tilings) and glds."""
    M, K, N = 4100, 128, 320
    lda = R.lda_at_span_limit(M) - (0 if where == "at_limit" else 8)
    assert (R.a_span_bytes_linear(M, lda) >= 1 << 31) == (where == "at_limit")
    case = lin_case(1000, M, N, K, True, 100, True)
    buf = torch.empty(M * lda, dtype=torch.float16, device=DEV)
    a = buf.view(M, lda)[:, :K]
    a.copy_(case["a"].to(DEV))
    pw = pack(case)
    for route in ("w80", "w80w", "glds160"):
        for k, v in R.ROUTES[route]["knobs"].items():
            tune(k, v)
        want = R.ROUTES["glds160" if where == "at_limit" else route]["sig"][0]
        assert ops.gemm_colsum_rows(a, pw, M=M) == want, f"{where}: {route} knobs report another kernel"
        if where == "at_limit" and route != "w80":     # (all three knob sets resolve to the 256-row kernel: one launch)
            continue
        out, obuf, _ = launch(route, case, a_dev=a, check_route=False)
        check(out, obuf, case, f"address range {where} (lda {lda}) {route} knobs", "H")
    del buf


# ---------------------------------------------------------------- I. query and launch agree
FLAGS = ("colsum", "rowsum", "lnfold", "ln")


def agree(route, case, seen, what, *, act=None, splits=1, out_f32=False):
    """One case of group C with each of COLSUM / ROWSUM / LNFOLD / LN: query 0 -> the launch with the flag returns MOCA_E_BADARG and
    writes nothing; non-zero -> it is accepted, every row is written and (the fold aside) the output is still right."""
    M = case["M"]
    pw = ops.finish_lnfold(pack(case, act=act))
    N, n_out = pw.N, (pw.n_out if act == "geglu" else pw.N)
    a = case["a"].to(DEV)
    res = case["res"].to(DEV) if case["res"] is not None else None
    radd = case["rowadd"].to(DEV) if case["rowadd"] is not None else None
    base = dict(M=M, residual=res, rowadd=radd, rowadd_div=case["div"], force_small=R.needs_force_small(route, M), splits=splits,
                out_f32=out_f32, gelu=(act == "gelu"))
    if splits > 1:
        base["splitk_ws"] = torch.full((splits * M * N,), NAN, dtype=torch.float32, device=DEV)
    af = a.float()
    part = torch.zeros(M + 512, 2, dtype=torch.float32, device=DEV)
    part[:M] = torch.stack([af.sum(1), (af * af).sum(1)], -1)
    one = torch.ones(N, dtype=torch.float32, device=DEV)
    odt = torch.float32 if out_f32 else torch.float16
    for flag in FLAGS:
        out = torch.full((M, n_out), NAN, dtype=odt, device=DEV)
        if flag == "colsum":
            q = ops.gemm_colsum_rows(a, pw, **base)
            kw = dict(colsum=torch.full(((M + 31) // 32, N, 2), NAN, dtype=torch.float32, device=DEV))
        elif flag == "rowsum":
            q = ops.gemm_rowsum_cols(a, pw, rowsum=True, **base)
            kw = dict(rowsum=torch.full(((N // 64 + 1) * M, 2), NAN, dtype=torch.float32, device=DEV))
        elif flag == "lnfold":
            q = ops.gemm_lnfold_ok(a, pw, lnfold=(None, 1, 1e-5), **base)
            kw = dict(lnfold=(part, 1, 1e-5))
        else:
            q = ops.gemm_ln_ok(a, pw, ln=(one, one, None, 1e-5), **base)
            kw = dict(ln=(one, one, torch.full((M, N), NAN, dtype=torch.float16, device=DEV), 1e-5))
        seen[flag] = seen.get(flag, 0) + bool(q)
        w = f"{what} {flag}: query {q}"
        if q:
            ops.gemm(a, pw, out, **base, **kw)
            assert torch.isfinite(out).all(), f"{w}, accepted, but rows were left unwritten"
            if flag != "lnfold":                       # (the fold changes what is computed: tests/test_kernels_gpu.py::test_gemm_rowsum_feeds_lnfold)
                R.check_blocks(out, case["ref"], w, tol=TOL32 if out_f32 else TOL16, group="I")
        else:
            with pytest.raises(L.MocaHipError):
                ops.gemm(a, pw, out, **base, **kw)
            torch.cuda.synchronize()
            assert torch.isnan(out).all(), f"{w}, refused, but the output was written"


@pytest.mark.parametrize("route", list(R.ROUTES))
def test_query_and_launch_agree(route, tune):
    """Every case of group C on this route -- bias x row add x residual at every M, rowadd_div in {1, 7, 100, M}, both column counts; then
    split-K through the reduce (splits = 2), fp32 output (splits 1 and 3), GELU, and GEGLU with splits 1 and 2 -- with each of COLSUM /
    ROWSUM / LNFOLD / LN (agree()).  The plain cases reach the accepted branch on the kernels that have the epilogue, the split-K / fp32 /
    GELU / GEGLU cases the refused branch on the same kernels (colsum_rows: splits != 1; rowsum_cols: OUT_F32 | GELU | ...)."""
    take(tune, route)
    tune(R.G4P, 0), tune(R.SQP, 0)
    spec = R.ROUTES[route]
    K = spec.get("K", 64)
    seen = {}
    for N in R.route_Ns(route):
        for M in spec["M"]:
            for bias, ra, rs in combos(route):
                for div in ((1, 7, 100, M) if ra else (0,)):
                    case = lin_case(200 + M, M, N, K, bool(bias), div, bool(rs))
                    agree(route, case, seen, f"{route} M={M} N={N} bias={bias} rowadd={ra}/{div} res={rs}")
    cs, rc, lf = spec["sig"]
    if route != "ws":                                  # the route's own statistics were accepted on some case, the others refused on all
        assert (seen["colsum"] > 0) == (cs > 0) and (seen["rowsum"] > 0) == (rc > 0) and (seen["lnfold"] > 0) == bool(lf), seen
    refused = {}
    N, M = spec["N"], spec["M"][-1]
    K3 = spec.get("K", 192)
    agree(route, lin_case(260 + M, M, N, K3, True, 7, True), refused, f"{route} M={M} splits=2", splits=2)
    for splits in (1, 3):
        agree(route, lin_case(300 + M + N, M, N, K3, True, 7, True), refused, f"{route} M={M} fp32 splits={splits}", splits=splits, out_f32=True)
    for Mg in (128, 129):
        agree(route, lin_case(400 + Mg + 64, Mg, N, 64, True, 0, False, "gelu"), refused, f"{route} M={Mg} gelu", act="gelu")
    assert not any(refused[f] for f in ("colsum", "rowsum", "ln")), f"split-K / fp32 / GELU carry no statistics epilogue: {refused}"
    geglu = {}
    for splits in (1, 2):
        agree(route, lin_case(450 + M, M, 256, 192, True, 0, False, "geglu"), geglu, f"{route} M={M} geglu splits={splits}", act="geglu", splits=splits)
    assert not any(geglu[f] for f in ("colsum", "rowsum", "ln")), f"GEGLU carries no statistics epilogue: {geglu}"
