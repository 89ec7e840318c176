"""The halo form of the 320 x 160 staggered kernel (csrc/gemm_halo.hip, MOCA_ROUTE_W80H, knob MOCA_TUNE_CONV_HALO): stride-1 3 x 3 convs
whose 320-row tiles are whole image rows of one frame read an LDS-resident halo tile instead of gathering every tap.

Reference: fp32 torch.nn.functional.conv2d per frame on the same fp16-rounded inputs and weights; bound: the single-kernel bound
3e-3 of max|ref|, against the reference and against the per-tap gather forced by the knob (not bit-identical: the fp32
summation order over k differs).  Every launch under test asserts through ops.gemm_route that the halo kernel takes it.

Geometries (W, H, frames) -- the smallest that can go wrong:
  (64, 5, 2)   one tile per frame: every halo row above / below is outside the image; with the OTHER frame NaN the output stays finite
  (64, 10, 3)  two tiles per frame: border and interior halo rows meet at the seam y = 4 / 5
  (32, 20, 2)  ten image rows per tile, two tiles per frame          (32, 10, 1)  the same geometry, one tile
Channels 32 (one slice), 96 (odd slice count: the slice pair has a tail), 320; N = 320 (two column tiles) and 640 (C = 320 only).  A single
column tile, N = 160, is not a call the library accepts: moca_gemm_f16 wants N % 64 == 0 and the 320 x 160 kernels N % 160 == 0.
GroupNorm statistics: equal to the gather's to the fixed-point unit (2^-20 / 2^-12), asserted as integer equality of the gstat buffers on
small-integer operands, where every partial sum is exact in fp32 whatever the k order and both kernels stage the same fp16 tile.  On
random operands the staged fp16 elements differ by the summation order; there the statistics are held to 1e-3 of the largest statistic
against the gather's and against the sums of the written output (the bound tests/test_gemm_edges_gpu.py asks of every statistics epilogue)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

DEV = "cuda"
TOL = 3e-3
NAN = float("nan")
GEOS = {"w64h5f2": (64, 5, 2), "w64h10f3": (64, 10, 3), "w32h20f2": (32, 20, 2), "w32h10f1": (32, 10, 1)}
CASES = [("w64h5f2", 32, 320), ("w64h5f2", 96, 320), ("w64h5f2", 320, 640), ("w64h10f3", 96, 320), ("w64h10f3", 320, 320),
         ("w32h20f2", 32, 320), ("w32h20f2", 96, 320), ("w32h20f2", 320, 640), ("w32h10f1", 96, 320), ("w32h10f1", 320, 320)]


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    ops.set_stream(None)
    torch.cuda.synchronize()


@pytest.fixture
def tune():
    saved = []

    def set_(knob, value):
        saved.append((knob, L.set_tuning(knob, value)))
    yield set_
    for knob, old in reversed(saved):
        L.set_tuning(knob, old)


def halo_on(tune):
    tune(L.MOCA_TUNE_GEMM_W80, 2)                       # (no tile-count rule: the test shapes have 2 to 12 tiles)
    tune(L.MOCA_TUNE_CONV_HALO, 1)


def ref_conv(x, w, b):
    """x fp16 [F][H][W][C], w fp16 [N][C][3][3], b fp32 [N] -> fp32 [F*H*W][N], frame by frame"""
    out = [F.conv2d(f.permute(2, 0, 1)[None].float(), w.float(), b.float(), padding=1)[0].permute(1, 2, 0) for f in x]
    return torch.stack(out).reshape(-1, w.shape[0])


@functools.lru_cache(maxsize=None)
def case(geo, Cn, N):
    """host operands and the reference, computed once and shared (never written to)"""
    W, H, Fr = GEOS[geo]
    g = torch.Generator().manual_seed(1000 * Cn + N + W + H)
    x = (torch.randn(Fr, H, W, Cn, generator=g)).half()
    w = (torch.randn(N, Cn, 3, 3, generator=g) / (3.0 * Cn ** 0.5)).half()
    b = torch.randn(N, generator=g)
    return x, w, b, ref_conv(x, w, b)


def conv_kw(geo, Cn):
    W, H, Fr = GEOS[geo]
    return dict(M=Fr * H * W, mode=L.MOCA_A_CONV3X3, conv=(Cn, H, W, H, W, 1, 0))


def launch(x, pw, geo, Cn, halo, **kw):
    """one launch into a NaN-poisoned output; asserts the route"""
    M = conv_kw(geo, Cn)["M"]
    out = torch.full((M, pw.N), NAN, dtype=torch.float16, device=DEV)
    old = L.set_tuning(L.MOCA_TUNE_CONV_HALO, 1 if halo else 0)
    try:
        route = ops.gemm_route(x, pw, out, **conv_kw(geo, Cn), **kw)
        assert (route == L.MOCA_ROUTE_W80H) == halo, f"{geo} C={Cn} N={pw.N}: route {route} with the halo knob at {int(halo)}"
        ops.gemm(x, pw, out, **conv_kw(geo, Cn), **kw)
    finally:
        L.set_tuning(L.MOCA_TUNE_CONV_HALO, old)
    torch.cuda.synchronize()
    return out


def close(got, ref, what):
    assert torch.isfinite(got).all(), f"{what}: rows left unwritten or not finite"
    err = ((got.float().cpu() - ref).abs().max() / ref.abs().max()).item()
    print(f"[halo] {what}: {err:.2e} of max|ref|")
    assert err <= TOL, f"{what}: {err:.2e} of max|ref| (bound {TOL:.0e})"


@pytest.mark.parametrize("geo,Cn,N", CASES)
def test_halo_conv_matches_conv2d_and_the_gather(tune, geo, Cn, N):
    halo_on(tune)
    x, w, b, ref = case(geo, Cn, N)
    xd, pw = x.to(DEV), ops.pack_conv3x3(w, b)
    got = launch(xd, pw, geo, Cn, True)
    close(got, ref, f"{geo} C={Cn} N={N} vs conv2d")
    old = launch(xd, pw, geo, Cn, False)
    close(got, old.float().cpu(), f"{geo} C={Cn} N={N} vs the gather")
    if geo == "w64h10f3":                                  # the rows on either side of the tile seam y = 4 / 5 of every frame
        W, H, Fr = GEOS[geo]
        rows = torch.cat([torch.arange(f * H * W + 4 * W, f * H * W + 6 * W) for f in range(Fr)])
        close(got[rows.to(DEV)], ref[rows], f"{geo} C={Cn} N={N} seam rows")


@pytest.mark.parametrize("nan_frame", [0, 1])
def test_no_tap_reads_across_a_frame(tune, nan_frame):
    halo_on(tune)
    geo, Cn, N = "w64h5f2", 96, 320
    x, w, b, ref = case(geo, Cn, N)
    xn = x.clone()
    xn[nan_frame] = NAN
    got = launch(xn.to(DEV), ops.pack_conv3x3(w, b), geo, Cn, True)
    W, H, _ = GEOS[geo]
    keep = slice((1 - nan_frame) * H * W, (2 - nan_frame) * H * W)
    close(got[keep], ref[keep], f"frame {1 - nan_frame} beside a NaN frame")
    assert torch.isnan(got[nan_frame * H * W:(nan_frame + 1) * H * W]).all()


@pytest.mark.parametrize("geo", ["w64h10f3", "w32h10f1"])
def test_border_columns(tune, geo):
    halo_on(tune)
    Cn, N = 96, 320
    x, w, b, _ = case(geo, Cn, N)
    xb = torch.zeros_like(x)
    xb[:, :, 0], xb[:, :, -1] = x[:, :, 0], x[:, :, -1]
    got = launch(xb.to(DEV), ops.pack_conv3x3(w, b), geo, Cn, True)
    close(got, ref_conv(xb, w, b), f"{geo} border columns")


def test_epilogues_residual_rowadd_statistics(tune):
    halo_on(tune)
    geo, Cn, N = "w64h10f3", 320, 320                   # (C % 64 == 0: the gather runs on the 320-row kernel too, same statistics tiles)
    W, H, Fr = GEOS[geo]
    M, HW = Fr * H * W, H * W
    x, w, b, ref = case(geo, Cn, N)
    xd, pw = x.to(DEV), ops.pack_conv3x3(w, b)
    g = torch.Generator().manual_seed(7)
    res, emb = torch.randn(M, N, generator=g).half(), torch.randn(Fr, N, generator=g).half()
    got = launch(xd, pw, geo, Cn, True, residual=res.to(DEV))
    close(got, ref + res.float(), "+res")
    got = launch(xd, pw, geo, Cn, True, rowadd=emb.to(DEV), rowadd_div=HW)
    close(got, ref + emb.float().repeat_interleave(HW, 0), "+rowadd")
    scale = torch.tensor([2.0 ** -20, 2.0 ** -12], dtype=torch.float64)
    stats = {}
    for halo in (True, False):
        gst = torch.zeros(M // 320 * 64, dtype=torch.int64, device=DEV)
        got = launch(xd, pw, geo, Cn, halo, rowadd=emb.to(DEV), rowadd_div=HW, gstat=(gst, 320))
        close(got, ref + emb.float().repeat_interleave(HW, 0), f"+gstat (halo {int(halo)})")
        stats[halo] = gst.cpu().view(M // 320, 32, 2).double() * scale
        xo = got.double().cpu().view(M // 320, 320, 32, N // 32)
        for j, own in enumerate((xo.sum((1, 3)), (xo * xo).sum((1, 3)))):
            e = ((stats[halo][..., j] - own).abs().max() / own.abs().max()).item()
            assert e <= 1e-3, f"gstat [{j}] (halo {int(halo)}) off its own output's sums by {e:.2e}"
    for j in range(2):
        e = ((stats[True][..., j] - stats[False][..., j]).abs().max() / stats[False][..., j].abs().max()).item()
        print(f"[halo] gstat [{j}] vs the gather: {e:.2e} of the largest statistic")
        assert e <= 1e-3, f"gstat [{j}]: halo and gather differ by {e:.2e}"
    rows = ops.gemm_colsum_rows(xd, pw, **conv_kw(geo, Cn))
    assert rows == 320
    cs = torch.full((M // rows, N, 2), NAN, dtype=torch.float32, device=DEV)
    got = launch(xd, pw, geo, Cn, True, colsum=cs)
    rt = got.double().cpu().view(M // rows, rows, N)
    want = torch.stack([rt.sum(1), (rt * rt).sum(1)], -1)
    e = ((cs.double().cpu() - want).abs().max() / want.abs().max()).item()
    assert e <= 2e-3, f"column sums off the output's by {e:.2e}"


def test_statistics_equal_the_gathers_to_the_fixed_point_unit_on_exact_operands(tune):
    """Small-integer inputs, weights, bias and row add: every partial sum is an integer below 2^24, exact in fp32 whatever the k order, so
    the halo kernel and the gather stage the SAME fp16 tile and their 64-bit fixed-point statistics must be equal to the unit (and the
    outputs bit for bit).  One dropped or doubled element of a group changes a sum by at least 2^20 units."""
    halo_on(tune)
    geo, Cn, N = "w64h10f3", 320, 320
    W, H, Fr = GEOS[geo]
    M, HW = Fr * H * W, H * W
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-2, 3, (Fr, H, W, Cn), generator=g).half()
    w = (torch.randint(-1, 2, (N, Cn, 3, 3), generator=g) * (torch.rand(N, Cn, 3, 3, generator=g) < 0.125)).half()
    b = torch.randint(-3, 4, (N,), generator=g).float()
    emb = torch.randint(-1, 2, (Fr, N), generator=g).half()
    ref = ref_conv(x, w, b) + emb.float().repeat_interleave(HW, 0)
    assert ref.abs().max() < 2048 and (ref != 0).float().mean() > 0.9          # exact in fp16, and not a trivial tile
    xd, pw = x.to(DEV), ops.pack_conv3x3(w, b)
    outs, stats = {}, {}
    for halo in (True, False):
        gst = torch.zeros(M // 320 * 64, dtype=torch.int64, device=DEV)
        outs[halo] = launch(xd, pw, geo, Cn, halo, rowadd=emb.to(DEV), rowadd_div=HW, gstat=(gst, 320)).cpu()
        stats[halo] = gst.cpu()
    assert torch.equal(outs[True].float(), ref), "halo output differs from the exact convolution"
    assert torch.equal(outs[True], outs[False]), "halo and gather outputs differ on exact operands"
    assert torch.equal(stats[True], stats[False]), \
        f"fixed-point statistics differ by up to {(stats[True] - stats[False]).abs().max().item()} units"
    want = ref.double().view(M // 320, 320, 32, N // 32)
    want = torch.stack([want.sum((1, 3)) * 2.0 ** 20, (want * want).sum((1, 3)) * 2.0 ** 12], -1).round().long().view(-1)
    assert torch.equal(stats[True], want), "fixed-point statistics differ from the exact sums"


def test_eager_capture_and_replay_are_bit_identical(tune):
    halo_on(tune)
    geo, Cn, N = "w32h20f2", 96, 320
    x, w, b, ref = case(geo, Cn, N)
    xd, pw = x.to(DEV), ops.pack_conv3x3(w, b)
    kw = conv_kw(geo, Cn)
    lib = L.load()
    st = torch.cuda.Stream()
    handle = C.c_void_p(st.cuda_stream)
    out = torch.full((kw["M"], N), NAN, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    ops.set_stream(st.cuda_stream)
    assert ops.gemm_route(xd, pw, out, **kw) == L.MOCA_ROUTE_W80H
    ops.gemm(xd, pw, out, **kw)
    st.synchronize()
    eager = out.clone()
    out.fill_(NAN)
    torch.cuda.synchronize()
    L.check(lib.moca_graph_begin(handle), "moca_graph_begin")
    try:
        ops.gemm(xd, pw, out, **kw)
    finally:
        graph = C.c_void_p()
        rc = lib.moca_graph_end(handle, C.byref(graph))
    assert rc == 0 and graph.value
    try:
        passes = []
        for _ in range(2):
            out.fill_(NAN)
            torch.cuda.synchronize()
            L.check(lib.moca_graph_launch(graph, handle), "moca_graph_launch")
            st.synchronize()
            passes.append(out.clone())
    finally:
        lib.moca_graph_destroy(graph)
    close(eager, ref, "eager pass")
    assert torch.equal(eager, passes[0]) and torch.equal(eager, passes[1]), "eager, first and second replay differ"


def test_refused_shapes_stay_on_the_gather(tune):
    halo_on(tune)
    t = torch.empty(1, 8, dtype=torch.float16, device=DEV)

    def route(Cn, H, W, oh, ow, stride, N=320, frames=2, **kw):
        pw = ops.PackedWeight(t, None, N, 9 * Cn, N)
        pw.w = torch.empty(1, (9 * Cn + 63) // 64 * 64, dtype=torch.float16, device=DEV)
        return ops.gemm_route(t, pw, t, M=frames * oh * ow, mode=L.MOCA_A_CONV3X3, conv=(Cn, H, W, oh, ow, stride, 0), **kw)

    assert route(64, 10, 64, 10, 64, 1) == L.MOCA_ROUTE_W80H
    assert route(64, 12, 48, 12, 48, 1) == L.MOCA_ROUTE_W80               # 320 % W != 0
    assert route(64, 7, 64, 7, 64, 1, frames=5) == L.MOCA_ROUTE_W80       # H % (320 / W) != 0
    assert route(64, 20, 64, 10, 32, 2) == L.MOCA_ROUTE_W80               # stride 2
    ws = torch.empty(8, dtype=torch.float32, device=DEV)
    assert route(64, 10, 64, 10, 64, 1, splits=2, splitk_ws=ws) == L.MOCA_ROUTE_W80
    L.set_tuning(L.MOCA_TUNE_CONV_HALO, 0)
    assert route(64, 10, 64, 10, 64, 1) == L.MOCA_ROUTE_W80
