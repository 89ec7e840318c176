"""Case tables, operands and float64 torch restatements for tests/test_gemm_fused_gpu.py and tests/test_gemm_fused_cpu.py: what
moca_gemm_f16 does beyond bias, row add, residual and GEGLU.

  A  MOCA_EP_LN       the LayerNorm store loop of the 160 x 320 tiling ............ ln_cases()
  B  MOCA_EP_LNFOLD   on every route that has it, synthetic row partials .......... fold_cases()
  C  a2 / k1 / lda2   the virtual torch.cat on the staggered kernels .............. cat_cases()
  D  wgroup_rows      per-row-group weights on w80, w80w and ws ................... wgroup_cases()
  E  MOCA_EP_GSTAT    one source of a virtual concat on the tiled routes .......... gstat_cases()
  F  MOCA_EP_TATTN    projection + temporal attention, plain / causal / folded .... tattn_cases()

A case is a dict; `route` names the kernel it is meant for (gemm_edges_ref.ROUTES / PERSISTENT, "tattn", or "refused").  build(case, dev)
draws the operands at scale 1 from the case's seed on the CPU, lays every operand into a larger NaN-filled allocation on `dev`
(lda = K + 8, ldo = N + 8, ld_ln = N + 16, ldr = N + 24, guard rows, canaries round every statistics buffer) and returns the keywords of
the ops.gemm call; reference(case, ops, wrong) restates the call in float64 on the same fp16 operands, `wrong` selecting one deliberately
wrong restatement (WRONGS: the CPU file asserts that each is at least 10 x the bound away).  Nothing here touches a GPU by itself: with
dev = "cpu" the same launch keywords answer the host queries."""
import itertools

import torch

import gemm_edges_ref as R
from gemm_edges_ref import NAN, TOL16, gen, randh
from moca_video_amd import lib as L

EPS = 1e-5
GSTAT_SCALE = (2.0 ** -20, 2.0 ** -12)          # include/moca_hip.h: the i64 accumulators' units (sum, sum of squares)
GSTAT_CANARY = -(1 << 62) + 12345               # (an i64 buffer has no NaN: a value no launch of these sizes can produce)
TOL_ROWSUM, TOL_COLSUM, TOL_GSTAT = 1e-4, 2e-3, 1e-3
# the row power of a unit-gamma, zero-beta LayerNorm row (mean of ln_out^2 = var / (var + eps)): every stored value carries one fp16
# rounding of at most 2^-11, its square twice that even if all 320 round the same way, plus 2^-13 for the fp32 statistics (generous);
# a variance over N - 1 moves it by 1 / N = 3.1e-3
TOL_ROWPOWER = 2.0 ** -10 + 2.0 ** -13
ROUTE_ID = dict(R.ROUTE_ID, tattn=L.MOCA_ROUTE_TATTN, refused=0)

WRONGS = {
    "A": ("ln_before_residual", "var_n_minus_1"),
    "B": ("second_partial_dropped", "padded_k"),
    "C": ("sources_exchanged", "k1_one_tile_late"),
    "D": ("group0_weights", "group0_bias"),
    "E": ("coff_ignored", "seam_to_left_neighbour"),
    "F": ("mask_transposed", "diagonal_masked", "pixels_16_19_take_19", "tile_row_statistics"),
}


def knobs_of(route):
    if route in R.ROUTES:
        return R.ROUTES[route]["knobs"]
    if route in R.PERSISTENT:
        return R.PERSISTENT[route]["knobs"]
    return {}


def case_knobs(c):
    """the knobs a case runs under: its route's, or those of the persistent kernel it must NOT run on (`under`)"""
    if c.get("under") in R.PERSISTENT:
        return knobs_of(c["under"])
    k = dict(knobs_of(c["route"]))
    if c["route"] == "g4":                              # (the GEGLU consumers: off the persistent kernels, as tests/test_gemm_edges_gpu.py)
        k.update({R.G4P: 0, R.SQP: 0})
    return k


def tile_rows(route):
    return R.ROUTE_TILE[ROUTE_ID[route]][0]


def tile_cols(route):
    return R.ROUTE_TILE[ROUTE_ID[route]][1]


def case_id(c):
    keys = ("M", "N", "K", "k1", "bias", "div", "res", "res_offset", "alias", "groups", "ln", "rowsum", "colsum", "gstat", "nparts",
            "geglu", "B", "HW", "heads", "causal", "regime", "under")
    return c["sec"] + "-" + c["route"] + "-" + "-".join(f"{k}{c[k]}" for k in keys if c.get(k) not in (None, False, 0, ""))


def _case(sec, route, M, N, K, seed, **kw):
    c = dict(sec=sec, route=route, M=M, N=N, K=K, seed=seed, bias=True, div=0, res=False, res_offset=0.0, alias=False, k1=0, groups=0,
             ln=None, rowsum=False, colsum=False, gstat=None, nparts=0, geglu=False, under=None, gap=0)
    c.update(kw)
    return c


# ---------------------------------------------------------------- case tables
def ln_cases():
    """A.  M = one tile + 1, two tiles, two tiles + 1, four tiles + 1 of the 160-row tile; bias x row add x residual with rowadd_div in
    {1, 7, M}; `out` aliasing `residual`; per-group weights (2 and 3 groups of one tile); residual rows offset by 40 and 100;
    gamma = 0; gamma = 1, beta = 0 (the row-power check)"""
    out = []
    for M in R.ROUTES["w80w"]["M"]:
        for K in R.FAST_KS:
            for b, ra, rs in itertools.product((1, 0), repeat=3):
                for div in ((1, 7, M) if ra else (0,)):
                    out.append(_case("A", "w80w", M, 320, K, 3000 + M + K, bias=bool(b), div=div, res=bool(rs), ln="std"))
    out.append(_case("A", "w80w", 321, 320, 64, 3001, div=7, res=True, alias=True, ln="std"))
    for M in (320, 480):
        out.append(_case("A", "w80w", M, 320, 64, 3002 + M, res=True, groups=M // 160, gap=64, ln="std"))
    for off in (40.0, 100.0):
        out.append(_case("A", "w80w", 321, 320, 64, 3003, res=True, res_offset=off, ln="std"))
    out.append(_case("A", "w80w", 321, 320, 64, 3004, res=True, div=7, ln="gamma0"))
    out.append(_case("A", "w80w", 321, 320, 192, 3005, res=True, ln="unit"))
    return out


FOLD_NPARTS = (1, 2, 3, 10)                     # the p0, p1, loop and maximum branches of lnfold_issue / lnfold_finish
FOLD_ROUTES = tuple(r for r, s in R.ROUTES.items() if s["sig"][2] is True)
FOLD_GEGLU = ("g4", "sq256", "g4p", "g4q", "sqp")


def fold_cases():
    """B.  The tiled routes at their M sets, K in (64, 192), every nparts, once with a bias and once with residual + row add (no bias);
    the second column count at nparts = 2; GEGLU consumers on g4 and the persistent kernels; the persistent kernels at their minimum
    shapes, plain (bias, then residual + row add) and GEGLU."""
    out = []
    for route in FOLD_ROUTES:
        spec = R.ROUTES[route]
        for M in spec["M"]:
            for K in R.FAST_KS:
                for nparts in FOLD_NPARTS:
                    out.append(_case("B", route, M, spec["N"], K, 4000 + M + K + nparts, nparts=nparts))
                    out.append(_case("B", route, M, spec["N"], K, 4100 + M + K + nparts, nparts=nparts, bias=False, res=True, div=7))
            out.append(_case("B", route, M, spec["N2"], 192, 4200 + M, nparts=2, res=True))
    for M in R.ROUTES["g4"]["M"]:
        for nparts in FOLD_NPARTS:
            out.append(_case("B", "g4", M, 256, 64 if nparts % 2 else 192, 4300 + M + nparts, nparts=nparts, geglu=True))
    for name, (M, N, K) in R.PERSISTENT_SHAPE.items():
        out.append(_case("B", name, M, N, K, 4400, nparts=1))
        out.append(_case("B", name, M, N, K, 4401, nparts=10, bias=False, res=True, div=7))
        out.append(_case("B", name, M, N, K, 4402, nparts=2, geglu=True))
        out.append(_case("B", name, M, N, K, 4403, nparts=3, geglu=True, bias=False))
    return out


CAT_KS = ((128, 64), (192, 64), (192, 128), (384, 320))
CAT_EPILOGUES = ("res_rowadd", "rowsum", "colsum", "gstat")
PERSISTENT_CAT = dict(M=13440, N=1280, K=128, k1=64)     # 265 / 530 tiles: the smallest shape sqp and g4p both accept (N % 160 == 0)


def _epi(e, route, M):
    if e == "res_rowadd":
        return dict(res=True, div=7)
    if e == "gstat":                            # (a row tile must lie inside one statistics group: where M is whole tiles)
        return dict(gstat=(tile_rows(route), 0, 0)) if M % tile_rows(route) == 0 else None
    return {e: True}


def cat_cases():
    """C.  w80 and w80w at their M sets and both column counts, (K, k1) with the seam after 1 / 2 / 5 k-tiles; residual + row add, row
    sums, column sums, GSTAT (where M is whole row tiles); under the persistent kernels' knobs the call stays on the staggered kernel"""
    out = []
    for route in ("w80", "w80w"):
        for N in R.route_Ns(route):
            for M in R.ROUTES[route]["M"]:
                for K, k1 in CAT_KS:
                    for e in CAT_EPILOGUES:
                        kw = _epi(e, route, M)
                        if kw is not None:
                            out.append(_case("C", route, M, N, K, 5000 + M + K + k1, k1=k1, **kw))
    for name in ("sqp", "g4p"):
        out.append(_case("C", "w80w", seed=5100, under=name, res=True, **PERSISTENT_CAT))
    return out


def wgroup_cases():
    """D.  2 and 3 groups of one and two row tiles on w80 / w80w, both column counts, K in (64, 192); 32-row strips on ws (2 groups of
    4096, 3 groups of 2752 = 86 strips); a gap of 64 NaN elements between the groups' matrices; residual, row sums, column sums and
    GSTAT with gstat_rows == wgroup_rows (the LayerNorm store loop on per-group weights: ln_cases)"""
    out = []
    for route in ("w80", "w80w"):
        tm = tile_rows(route)
        for N in R.route_Ns(route):
            for groups, mult in itertools.product((2, 3), (1, 2)):
                M = groups * mult * tm
                for K in R.FAST_KS:
                    for kw in (dict(res=True), dict(rowsum=True), dict(colsum=True), dict(gstat=(mult * tm, 0, 0), res=True)):
                        out.append(_case("D", route, M, N, K, 6000 + M + K, groups=groups, gap=64, **kw))
    for groups, rows in ((2, 4096), (3, 2752)):
        for kw in (dict(res=True), dict(rowsum=True), dict(gstat=(rows, 0, 0), res=True), dict()):
            out.append(_case("D", "ws", groups * rows, 320, 320, 6100 + rows, groups=groups, gap=64, **kw))
    return out


GSTAT_ROUTES = ("glds128", "glds160", "w80", "w80w")


def gstat_cpg_coff(N):
    """(cpg, coff) per column count: the default; the 960-channel concat at N = 320 (first and second source); the 1920-channel concat
    at N = 640; the last admissible group, (coff + N - 1) / cpg == 31, with seams inside the column tiles"""
    out = [(0, 0)]
    if N == 320:
        out += [(30, 0), (30, 640)]
    if N == 640:
        out += [(60, 1280)]
    cpg = N // 32 + 3
    out.append((cpg, 32 * cpg - N))
    assert (out[-1][1] + N - 1) // cpg == 31
    return out


def gstat_cases():
    """E.  gstat_rows = one and two row tiles, 2 and 3 statistics groups, both column counts, residual on every second case"""
    out = []
    for route in GSTAT_ROUTES:
        tm = tile_rows(route)
        for N in R.route_Ns(route):
            for groups, mult in itertools.product((2, 3), (1, 2)):
                for i, (cpg, coff) in enumerate(gstat_cpg_coff(N)):
                    out.append(_case("E", route, groups * mult * tm, N, 64 if (groups + i) % 2 else 192, 7000 + N + groups + mult + i,
                                     gstat=(mult * tm, cpg, coff), res=bool(i % 2)))
    return out


TATTN_SHAPES = ((1, 20, 1, 64), (3, 20, 2, 192), (2, 60, 5, 320))
TATTN_REFUSED = (1, 40, 2, 72)                  # K % 64 != 0: the staggered kernel's gather takes whole k-tiles (fast_gather)


def tattn_cases():
    """F.  smallest launch; one tile per video with batch stepping; three tiles per video.  Plain and causal x (no fold, fold with
    nparts 1 / 2 / 3, fold with a bias); a peaked regime (q x 6); causal again serves the frame-0 check.  K = 72 is refused."""
    out = []
    for (B, HW, heads, K), causal in itertools.product(TATTN_SHAPES, (False, True)):
        base = dict(sec="F", route="tattn", B=B, HW=HW, heads=heads, K=K, M=B * 16 * HW, N=192 * heads, causal=causal, seed=8000 + HW + K,
                    nparts=0, bias=False, regime="")
        out.append(dict(base))
        for nparts in (1, 2, 3):
            out.append(dict(base, nparts=nparts))
        out.append(dict(base, nparts=1, bias=True))
        out.append(dict(base, regime="peaked", nparts=2 if causal else 0))
    B, HW, heads, K = TATTN_REFUSED
    out.append(dict(sec="F", route="refused", B=B, HW=HW, heads=heads, K=K, M=B * 16 * HW, N=192 * heads, causal=False, seed=8100, nparts=0,
                    bias=False, regime=""))
    return out


SECTIONS = {"A": ln_cases, "B": fold_cases, "C": cat_cases, "D": wgroup_cases, "E": gstat_cases, "F": tattn_cases}


def all_cases():
    return [c for f in SECTIONS.values() for c in f()]


# ---------------------------------------------------------------- operands (CPU, seeded)
FOLD_CONST_ROW, FOLD_BIG = 3, (64, 128)         # a constant row (variance clamped at 0); one 64-row block with |mean| / std = 100
FOLD_BIG_RATIO = 100.0
FOLD_BIG_RATIO_GEGLU = 60.0                     # (value x gelu(gate) doubles the relative error: at 100 the fp32 slack reaches TOL16)


def distinct_rows(g, M, K, big=FOLD_BIG_RATIO):
    """every row its own mean (m mod 17) - 8 and standard deviation 0.5 .. 3 by (m mod 5): statistics of another row are an O(1) error"""
    m = torch.arange(M)
    mean, std = ((m % 17) - 8).float(), 0.5 + 0.625 * (m % 5).float()
    if big:
        lo, hi = FOLD_BIG
        hi = min(hi, M)
        if lo < M:
            std[lo:hi] = 1.0
            mean[lo:hi] = big
    x = (mean[:, None] + std[:, None] * torch.randn(M, K, generator=g)).half()
    if big and M > FOLD_CONST_ROW:
        x[FOLD_CONST_ROW] = 2.5
    return x


def row_partials(x, nparts):
    """f32 [nparts][M][2]: float64 sums / sums of squares of x over nparts column ranges"""
    xd = x.double()
    parts = [torch.stack([c.sum(1), (c * c).sum(1)], -1) for c in torch.tensor_split(xd, nparts, dim=1)]
    return torch.stack(parts).float()


def operands(c):
    """the fp16 / f32 operands of a linear case (sections A .. E), on the CPU"""
    g = gen(c["seed"])
    M, N, K = c["M"], c["N"], c["K"]
    G = max(c["groups"], 1)
    o = dict(a=distinct_rows(g, M, K, FOLD_BIG_RATIO_GEGLU if c["geglu"] else FOLD_BIG_RATIO) if c["nparts"] else randh(g, M, K))
    o["w"] = [randh(g, N, K, scale=K ** -0.5) for _ in range(G)]
    # column statistics: every column's bias is 0.5 + 0.25 per weight group, with a spread of 0.05 only, so that the plain sum of every
    # (statistics group, channel group) pair -- down to one column of a seam group -- is far from zero and has a relative error
    o["b"] = None
    if c["bias"] and (c["colsum"] or c["gstat"]):
        o["b"] = [torch.randn(N, generator=g) * 0.05 + 0.5 + 0.25 * gi for gi in range(G)]
    elif c["bias"]:
        o["b"] = [torch.randn(N, generator=g) * (0.1 if c["geglu"] else 1.0) for _ in range(G)]
    o["ra"] = randh(g, (M + c["div"] - 1) // c["div"], c["N"]) if c["div"] else None
    o["res"] = (torch.randn(M, N, generator=g) + c["res_offset"]).half() if c["res"] else None
    if c["ln"]:
        o["gamma"] = {"std": torch.randn(N, generator=g) * 0.2 + 1.0, "gamma0": torch.zeros(N), "unit": torch.ones(N)}[c["ln"]]
        o["beta"] = torch.zeros(N) if c["ln"] == "unit" else torch.randn(N, generator=g) * 0.2
    if c["nparts"]:
        o["fg"], o["fb"] = torch.randn(K, generator=g) * 0.3 + 1.0, torch.randn(K, generator=g) * 0.3
        o["part"] = row_partials(o["a"], c["nparts"])
    return o


def layernorm64(y, gamma, beta, eps=EPS, ddof=0):
    mean = y.mean(1, keepdim=True)
    var = ((y - mean) ** 2).sum(1, keepdim=True) / (y.shape[1] - ddof)
    return (y - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def stats_from_partials(part, K, drop_second=False):
    """(mean, var) float64 [M] as the fold's epilogue derives them from the f32 partials: var = q / K - mean^2, clamped at 0"""
    p = part.double()
    if drop_second and p.shape[0] > 1:
        p = torch.cat([p[:1], p[2:]])
    s, q = p[..., 0].sum(0), p[..., 1].sum(0)
    mean = s / K
    return mean, (q / K - mean * mean).clamp_min(0.0)


def reference(c, o, wrong=None):
    """float64 restatement of a linear case -> dict(out [M][n_out], ln [M][N] or None); `wrong`: one of WRONGS"""
    M, N, K = c["M"], c["N"], c["K"]
    G = max(c["groups"], 1)
    a = o["a"].double()
    if c["k1"]:
        k1 = c["k1"]
        if wrong == "sources_exchanged":
            a = torch.cat([a[:, k1:], a[:, :k1]], 1)
        elif wrong == "k1_one_tile_late":              # the second source starts one k-tile late
            a = torch.cat([a[:, :k1], torch.zeros(M, 64, dtype=torch.float64), a[:, k1:K - 64]], 1)
    if c["nparts"]:
        if wrong in ("second_partial_dropped", "padded_k"):
            mean, var = stats_from_partials(o["part"], K + (8 if wrong == "padded_k" else 0), wrong == "second_partial_dropped")
            a = (a - mean[:, None]) / torch.sqrt(var[:, None] + EPS) * o["fg"].double() + o["fb"].double()
        else:
            a = layernorm64(a, o["fg"], o["fb"])
    rows = M // G
    ys = []
    for gi in range(G):
        wi = 0 if wrong == "group0_weights" else gi
        bi = 0 if wrong == "group0_bias" else gi
        y = a[gi * rows:(gi + 1) * rows] @ o["w"][wi].double().T
        ys.append(y + o["b"][bi].double() if o["b"] is not None else y)
    y = torch.cat(ys)
    pre = R.epilogue(y, None, o["ra"], max(c["div"], 1), None)
    y = R.epilogue(pre, None, None, 1, o["res"], "geglu" if c["geglu"] else None)
    ln = None
    if c["ln"]:
        ln = layernorm64(pre if wrong == "ln_before_residual" else y, o["gamma"], o["beta"], ddof=1 if wrong == "var_n_minus_1" else 0)
    return dict(out=y, ln=ln)


def wrongs_of(c):
    """the wrong restatements that apply to a case"""
    out = []
    if c["sec"] == "F":
        if c["route"] == "refused":
            return out
        out.append("pixels_16_19_take_19")
        if c["causal"]:
            out += ["mask_transposed", "diagonal_masked"]
        if c["nparts"]:
            out.append("tile_row_statistics")
        if c["nparts"] > 1:
            out.append("second_partial_dropped")
        return out
    if c["ln"] in ("std", "unit"):
        out.append("var_n_minus_1")
        if c["res"]:
            out.append("ln_before_residual")
    if c["nparts"]:
        out.append("padded_k")
        if c["nparts"] > 1:
            out.append("second_partial_dropped")
    if c["k1"]:
        out += ["sources_exchanged", "k1_one_tile_late"]
    if c["groups"]:
        out.append("group0_weights")
        if c["bias"]:
            out.append("group0_bias")
    if c["gstat"]:
        cpg, coff = c["gstat"][1:]
        if coff:
            out.append("coff_ignored")
        if cpg and (coff % cpg or (coff + c["N"]) % cpg):
            out.append("seam_to_left_neighbour")
    return out


def gstat_expected(c, y, wrong=None):
    """float64 [n_sg][32][2]: sums / sums of squares of the reference output per (statistics group, channel group); untouched groups 0"""
    rows, cpg, coff = c["gstat"]
    N = c["N"]
    cw = cpg if cpg else N // 32
    if wrong == "coff_ignored":
        coff = 0
    grp = (coff + torch.arange(N)) // cw
    if wrong == "seam_to_left_neighbour":
        for seam in {int(grp[0]) if coff % cw else None, int(grp[-1]) if (coff + N) % cw else None} - {None}:
            grp = torch.where(grp == seam, grp - 1, grp).clamp_min(0)
    yg = y.view(c["M"] // rows, rows, N)
    want = torch.zeros(c["M"] // rows, 32, 2, dtype=torch.float64)
    want[:, :, 0].index_add_(1, grp, yg.sum(1))
    want[:, :, 1].index_add_(1, grp, (yg * yg).sum(1))
    return want


def pair_errors(got, want):
    """relative error of every touched (statistics group, channel group) accumulator -> (worst, untouched pairs all exactly 0)"""
    touched = want[..., 1] > 0
    e = ((got - want).abs() / want.abs().clamp_min(1e-30))[touched]
    return e.max().item(), bool((got[~touched] == 0).all())


# ---------------------------------------------------------------- the fp32 restatement of the formulas that lose digits by design
def fold_fp32(c, o):
    """MOCA_EP_LNFOLD as csrc/gemm_device.h computes it, in fp32 torch: single-pass variance from the f32 partials,
    rstd * acc + (-mean * rstd * wsum + bias) on the folded fp16 weights -> [M][n_out] f32"""
    from moca_video_amd import ops
    K = c["K"]
    wf, bf = ops.fold_layernorm(o["w"][0], o["b"][0] if o["b"] is not None else None, o["fg"], o["fb"])
    wf = wf.half().float()
    s, q = o["part"][..., 0].sum(0), o["part"][..., 1].sum(0)
    inv_k = torch.tensor(1.0 / K, dtype=torch.float32)
    mean = s * inv_k
    rs = torch.rsqrt((q * inv_k - mean * mean).clamp_min(0.0) + EPS)
    y = rs[:, None] * (o["a"].float() @ wf.T) + ((-mean * rs)[:, None] * wf.sum(1)[None, :] + bf[None, :])
    y = R.epilogue(y, None, o["ra"].float() if o["ra"] is not None else None, max(c["div"], 1), o["res"].float() if o["res"] is not None else None)
    if c["geglu"]:
        inner = y.shape[1] // 2
        y = y[:, :inner] * torch.nn.functional.gelu(y[:, inner:])
    return y


def ln_fp32(c, o):
    """the two-pass LayerNorm of the store loop in fp32 torch on the fp32 linear + row add + residual -> [M][N] f32"""
    y = o["a"].float() @ o["w"][0].float().T + (o["b"][0] if o["b"] is not None else 0.0)
    y = R.epilogue(y, None, o["ra"].float() if o["ra"] is not None else None, max(c["div"], 1), o["res"].float() if o["res"] is not None else None)
    mean = y.mean(1, keepdim=True)
    d = y - mean
    return d * torch.rsqrt((d * d).mean(1, keepdim=True) + EPS) * o["gamma"] + o["beta"]


def block_tol(c, o, ref):
    """per 64-row block bound of the output whose formula loses digits at large row means (B: `out`; A: `ln_out`): TOL16, plus twice
    the block error of the fp32 restatement against float64 on the blocks with a large mean -> (tol [blocks], the slack [blocks])"""
    nb = (c["M"] + 63) // 64
    slack = torch.zeros(nb, dtype=torch.float64)
    if c["nparts"] and c["sec"] == "B" and c["M"] > FOLD_BIG[0]:
        b = FOLD_BIG[0] // 64
        slack[b] = 2 * R.block_errors(fold_fp32(c, o), ref["out"])[b]
    elif c["ln"] and c["res_offset"]:
        slack = 2 * R.block_errors(ln_fp32(c, o), ref["ln"])
    return TOL16 + slack, slack


# ---------------------------------------------------------------- one launch (sections A .. E)
def _canary_f32(n_rows, cols, dev, guard):
    buf = torch.full((n_rows + 2 * guard, cols), NAN, dtype=torch.float32, device=dev)
    return buf, buf[guard:guard + n_rows]


def build(c, o, dev):
    """lay the operands of a linear case out on `dev` -> dict(a, pw, out, kw = the keywords of ops.gemm / the queries, plus every canaried
    buffer).  A: [M + 2][K + 8] (two sources: k1 + 8 and K - k1 + 16), NaN outside; out ld N + 8, ln_out ld N + 16, residual ld N + 24."""
    from moca_video_amd import ops
    M, N, K = c["M"], c["N"], c["K"]
    G = max(c["groups"], 1)
    t = dict(c=c)
    kw = dict(M=M)
    if c["k1"]:
        k1 = c["k1"]
        _, t["a"] = R.embed(o["a"][:, :k1].contiguous(), pad=8, dev=dev)
        _, a2 = R.embed(o["a"][:, k1:].contiguous(), pad=16, dev=dev)
        kw["a2"] = (a2, k1)
    else:
        _, t["a"] = R.embed(o["a"], pad=8, dev=dev)
    # weights: per group packed on the CPU, laid `gap` NaN elements apart
    pws = []
    for gi in range(G):
        w, b = o["w"][gi], (o["b"][gi] if o["b"] is not None else None)
        if c["nparts"]:
            w, b = ops.fold_layernorm(w, b, o["fg"], o["fb"])
        pws.append((ops.pack_geglu if c["geglu"] else ops.pack_linear)(w, b, device="cpu"))
    p0 = pws[0]
    ldw = p0.w.stride(0)
    stride = p0.N * ldw + c["gap"]
    wbuf = torch.full((G * stride,), NAN, dtype=torch.float16)
    for gi, p in enumerate(pws):
        wbuf[gi * stride:gi * stride + p0.N * ldw] = p.w.reshape(-1)
    wbuf = wbuf.to(dev)
    bias = torch.cat([p.bias for p in pws]).to(dev) if p0.bias is not None else None
    pw = ops.PackedWeight(wbuf[:p0.N * ldw].view(p0.N, ldw), bias, p0.N, p0.K, p0.n_out, p0.geglu)
    if c["nparts"]:
        ops.finish_lnfold(pw)
    if c["groups"]:
        kw["wgroup"] = (M // G, stride)
    t["pw"], n_out = pw, (p0.n_out if c["geglu"] else p0.N)
    t["obuf"], t["out"] = R.canary_out(M, n_out, dev, pad=8)
    if c["res"]:
        if c["alias"]:
            t["out"].copy_(o["res"].to(dev))
            kw["residual"] = t["out"]
        else:
            kw["residual"] = R.embed(o["res"], pad=24, dev=dev)[1]
    if c["div"]:
        kw["rowadd"], kw["rowadd_div"] = R.embed(o["ra"], pad=8, dev=dev)[1], c["div"]
    if c["ln"]:
        t["lnbuf"], t["ln"] = R.canary_out(M, N, dev, pad=16)
        kw["ln"] = (o["gamma"].to(dev), o["beta"].to(dev), t["ln"], EPS)
    if c["rowsum"]:
        cols = tile_cols(c["route"])
        t["rsbuf"], part = _canary_f32(N // cols * M, 2, dev, 512)
        kw["rowsum"] = t["rs"] = part
    if c["colsum"]:
        tm = tile_rows(c["route"])
        t["csbuf"], t["cs"] = _canary_f32((M + tm - 1) // tm, 2 * N, dev, 1)
        kw["colsum"] = t["cs"]
    if c["gstat"]:
        rows, cpg, coff = c["gstat"]
        t["gsbuf"] = torch.full((M // rows + 2, 32, 2), GSTAT_CANARY, dtype=torch.int64, device=dev)
        t["gs"] = t["gsbuf"][1:-1]
        t["gs"].zero_()
        kw["gstat"] = (t["gs"], rows, cpg, coff) if (cpg or coff) else (t["gs"], rows)
    if c["nparts"]:
        t["pbuf"] = torch.full((c["nparts"] * M + 2, 2), NAN, dtype=torch.float32, device=dev)       # (a read past the partials is NaN)
        t["pbuf"][1:-1] = o["part"].view(-1, 2).to(dev)
        kw["lnfold"] = (t["pbuf"][1:-1], c["nparts"], EPS)
    t["kw"] = kw
    return t


def feature_ok(t):
    """the `_ok` queries of the features the case carries -> {query name: answer}"""
    from moca_video_amd import ops
    c, kw = t["c"], dict(t["kw"])
    out = {}
    if c["ln"]:
        out["ln_ok"] = ops.gemm_ln_ok(t["a"], t["pw"], **kw)
    if c["nparts"]:
        out["lnfold_ok"] = ops.gemm_lnfold_ok(t["a"], t["pw"], **kw)
    if c["k1"]:
        out["cat_ok"] = ops.gemm_cat_ok(t["a"], t["pw"], **kw)
    if c["groups"]:
        out["wgroup_ok"] = ops.gemm_wgroup_ok(t["a"], t["pw"], **kw)
    if c["rowsum"]:
        out["rowsum_cols"] = ops.gemm_rowsum_cols(t["a"], t["pw"], **kw) == tile_cols(c["route"])
    if c["colsum"] or c["gstat"]:
        out["colsum_rows"] = ops.gemm_colsum_rows(t["a"], t["pw"], **{k: v for k, v in kw.items() if k != "colsum"}) == tile_rows(c["route"])
    return out


# ---------------------------------------------------------------- F. MOCA_EP_TATTN
T_FRAMES, TATTN_SCALE, PEAK_GAIN = 16, 0.125, 6.0


def tattn_operands(c):
    g = gen(c["seed"] + 7 * c["nparts"] + (1 if c["bias"] else 0))
    M, K, C = c["M"], c["K"], 64 * c["heads"]
    o = dict(x=distinct_rows(g, M, K, big=0.0) if c["nparts"] else randh(g, M, K))
    o["wq"], o["wk"], o["wv"] = (randh(g, C, K, scale=K ** -0.5 * (PEAK_GAIN if (c["regime"] == "peaked" and i == 0) else 1.0)) for i in range(3))
    if c["nparts"]:
        o["fg"] = torch.randn(K, generator=g) * 0.3 + 1.0
        o["fb"] = torch.randn(K, generator=g) * 0.3 if c["bias"] else torch.zeros(K)
        o["part"] = row_partials(o["x"], c["nparts"])
    return o


def tile_row_of(B, HW):
    """global row -> the row whose statistics an un-gathered epilogue would take: tile row tr of tile t reads row 320 t + tr instead
    of grow(tr) = (16 b + (tr & 15)) HW + 20 pb + (tr >> 4) (csrc/gemm_w80s_kernel.inc)"""
    tpv = HW // 20
    idx = torch.empty(B * 16 * HW, dtype=torch.long)
    for t in range(B * tpv):
        b, pb = divmod(t, tpv)
        tr = torch.arange(320)
        idx[(16 * b + (tr & 15)) * HW + 20 * pb + (tr >> 4)] = 320 * t + tr
    return idx


def tattn_reference(c, o, wrong=None, unfolded=False):
    """float64 projection, rounded to fp16 as the epilogue stages it, then float64 softmax attention over the frame axis ->
    dict(out [M][C], v [M][C] = the staged v projection).  Under the fold the projection is restated on the fp16 operands the kernel
    reads -- normalise(x) @ W'^T + b' with W' = fp16(W diag(gamma)), b' = W beta (ops.fold_layernorm, before the per-head packing) --
    unless `unfolded`: Linear(LayerNorm(x)) with W itself.  The two differ by the rounding of W', 2^-11 per weight, which the peaked
    regime amplifies past TOL16 on the reference side alone (tests/test_gemm_fused_cpu.py::test_tattn_restatements_agree)."""
    from moca_video_amd import ops
    B, HW, heads, K, M = c["B"], c["HW"], c["heads"], c["K"], c["M"]
    T, C = T_FRAMES, 64 * heads
    a = o["x"].double()
    ws, bias = (o["wq"], o["wk"], o["wv"]), 0.0
    if c["nparts"]:
        one, zero = torch.ones(K), torch.zeros(K)
        if wrong in ("tile_row_statistics", "second_partial_dropped"):
            mean, var = stats_from_partials(o["part"], K, wrong == "second_partial_dropped")
            if wrong == "tile_row_statistics":
                idx = tile_row_of(B, HW)
                mean, var = mean[idx], var[idx]
            a = (a - mean[:, None]) / torch.sqrt(var[:, None] + EPS)
        else:
            a = layernorm64(a, one, zero)
        if unfolded:
            a = a * o["fg"].double() + o["fb"].double()
        else:
            wf, bf = ops.fold_layernorm(torch.cat(ws), None, o["fg"], o["fb"])
            ws, bias = wf.half().split(C), bf.double().split(C)
    q, k, v = ((a @ w.double().T + (bias[i] if c["nparts"] and not unfolded else 0.0)).half().double() for i, w in enumerate(ws))
    f = lambda t: t.view(B, T, HW, heads, 64).permute(0, 2, 3, 1, 4)                              # [B][HW][heads][T][64]
    s = torch.einsum("bphid,bphjd->bphij", f(q), f(k)) * TATTN_SCALE
    if c["causal"]:
        above = torch.ones(T, T).triu(1) > 0.5                                                    # key frame j > query frame i
        mask = above.T if wrong == "mask_transposed" else (torch.ones(T, T).triu(0) > 0.5 if wrong == "diagonal_masked" else above)
        s = s.masked_fill(mask, -1e30)
    out = (s.softmax(-1) @ f(v)).permute(0, 3, 1, 2, 4).reshape(B, T, HW, C)
    if wrong == "pixels_16_19_take_19":
        ot = out.view(B, T, HW // 20, 20, C).clone()
        ot[:, :, :, 16:19] = ot[:, :, :, 19:20]
        out = ot.view(B, T, HW, C)
    return dict(out=out.reshape(M, C), v=v)


def pixel_errors(got, ref, c):
    """max|got - ref| / max|ref| per pixel-within-tile 0..19 -> [20]"""
    sh = (c["B"], T_FRAMES, c["HW"] // 20, 20, -1)
    g, r = got.double().cpu().reshape(sh), ref.double().reshape(sh)
    return (g - r).abs().amax((0, 1, 2, 4)) / r.abs().amax((0, 1, 2, 4)).clamp_min(1e-30)


def tattn_errors(got, ref, c):
    """the worst (video, head) slice and the worst pixel-within-tile"""
    from attention_edges_ref import slice_errors
    return max(slice_errors(got.cpu(), ref, c["B"], c["heads"]).max().item(), pixel_errors(got, ref, c).max().item())


def tattn_build(c, o, dev):
    from moca_video_amd import ops
    heads, C, M, K = c["heads"], 64 * c["heads"], c["M"], c["K"]
    t = dict(c=c)
    kw = dict(M=M, tattn=(T_FRAMES, c["HW"], TATTN_SCALE, c["causal"]))
    if c["nparts"]:
        wf, bf = ops.fold_layernorm(torch.cat([o["wq"], o["wk"], o["wv"]]), None, o["fg"], o["fb"])
        pw = ops.finish_lnfold(ops.pack_qkv_per_head(wf[:C], wf[C:2 * C], wf[2 * C:], heads, bias=bf if c["bias"] else None, device=dev))
        t["pbuf"] = torch.full((c["nparts"] * M + 2, 2), NAN, dtype=torch.float32, device=dev)
        t["pbuf"][1:-1] = o["part"].view(-1, 2).to(dev)
        kw["lnfold"] = (t["pbuf"][1:-1], c["nparts"], EPS)
    else:
        pw = ops.pack_qkv_per_head(o["wq"], o["wk"], o["wv"], heads, device=dev)
    _, t["a"] = R.embed(o["x"], pad=8, dev=dev)
    t["pw"] = pw
    t["obuf"], t["out"] = R.canary_out(M, C, dev, pad=8)
    t["kw"] = kw
    return t
