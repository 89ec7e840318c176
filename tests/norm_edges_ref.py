"""Cases, float64 references, metric and wrong restatements of tests/test_norm_edges_cpu.py and tests/test_norm_edges_gpu.py: the
GroupNorm family of csrc/norm.hip (moca_groupnorm_nhwc_f16 on every route, moca_groupnorm_gstat_f16, moca_groupnorm_colsum_f16,
moca_groupnorm_gstat_cat_f16, moca_concat_channels_gstat_f16, moca_gstat_accum_f16, moca_groupnorm_fold_weights_f16).

Route and chunk geometry of a case come from the library's own queries (ops.groupnorm_route, ops.groupnorm_nchunk: the launch decides
with the same function); `route_restated` / `nchunk_restated` exist only to be compared with them.

Reference: two-pass float64 GroupNorm(32) (+SiLU) of the fp16 tensor as the kernel reads it (`reference`); for the statistics
producers exact sums (`stats_sums`: float64 sums of fp16 values; on the exact grids they are integers in the accumulators' units).

Metric: per (statistics group, channel group) block max|got - ref| / max|ref| of the same block (`block_errors`), every block within the
project's TOL16 = 3e-3 -- the per-block form of gemm_edges_ref, no new tolerance.

Inputs.  *Spike probes*: noise of std 0.05 around a small per-channel-group offset, plus ONE row per statistics group that carries
+-6 / 8 / 10 (sign and size by channel group, times 1 / 1.5 / 0.75 / 1.25 by statistics group) on all channels.  The row sits at another edge position in every statistics group
(`positions`: chunk, trip, remainder, split, frame and register-chunk edges); where a case has fewer statistics groups than positions
it runs several ROUNDS, each a launch of its own.  A row dropped from or counted twice in the statistics changes that group's rstd by a
factor; sign and size by group make a wrong channel grouping or a dropped SiLU an O(1) error too.  *Exact grids*: multiples of 1/8,
|x| <= 4: every partial sum is exact in fp32 while (rows of a partial) x cpg x 1024 < 2^24 (`grid_exact`), so the i64 accumulators
must EQUAL sum(x) 2^20 and sum(x^2) 2^12.

`restated(case, inp, wrong)` is the sums-based restatement with one of MUTATIONS applied; the CPU file shows that every case tells
every mutation that applies to it from the reference.

The launches of a case on guarded operands (`run_case`, `accumulate`, `fold_run`) live here too: tests/test_norm_edges_gpu.py judges what
they leave against the references above, tests/test_norm_parent_gpu.py and tools/record_parent_fixtures.py --norm-sha hash it
(`parent_hashes`).
"""
import zlib

import torch

from moca_video_amd import lib as L
from moca_video_amd import ops

TOL16 = 3e-3                    # tests/test_kernels_gpu.py: one fp16-output kernel against torch on the same fp16 operands
GROUPS = 32
EPS = 1e-5
SUM_SCALE, SQ_SCALE = 1 << 20, 1 << 12          # csrc/common.h MOCA_GSTAT_SUM_SCALE / MOCA_GSTAT_SQ_SCALE
SENTINEL = -777.0               # fp16-representable, far outside every output of the suite

ROUTE_ID = {"stream": L.MOCA_GN_ROUTE_STREAM, "slab2": L.MOCA_GN_ROUTE_SLAB2, "slab4": L.MOCA_GN_ROUTE_SLAB4, "slab8": L.MOCA_GN_ROUTE_SLAB8,
            "slabreg1": L.MOCA_GN_ROUTE_SLABREG1, "slabreg2": L.MOCA_GN_ROUTE_SLABREG2, "slabreg3": L.MOCA_GN_ROUTE_SLABREG3,
            "slabreg4": L.MOCA_GN_ROUTE_SLABREG4}
ROUTE_NAME = {v: k for k, v in ROUTE_ID.items()}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ----------------------------------------------------------------------------------------------------------------- restated dispatch
def nchunk_restated(F, HW):
    """gn_nchunk of csrc/norm.hip -- compared with ops.groupnorm_nchunk, never trusted"""
    if F <= 0 or HW <= 0:
        return 0
    return max(min(max(2048 // F, 1), (HW + 7) // 8), 1)


def route_restated(F, HW, C, fps, knob):
    """gn_plan of csrc/norm.hip under MOCA_TUNE_GN_SLAB = knob -- compared with ops.groupnorm_route, never trusted"""
    if F <= 0 or HW <= 0 or C <= 0 or C % 8 or C % GROUPS or fps <= 0 or F % fps or C // 8 > 1024:
        return 0
    cpg, nbytes, R = C // GROUPS, F * HW * C * 2, fps * HW
    if knob and cpg % 2 == 0 and cpg <= 128 and R < (1 << 24) and (knob == 2 or nbytes <= (8 << 20) or (fps == 1 and HW <= 160 and nbytes <= (28 << 20))):
        nchunks = R * (cpg // 8)
        if cpg % 8 == 0 and 256 <= nchunks <= 4096:
            return L.MOCA_GN_ROUTE_SLABREG1 + (nchunks + 1023) // 1024 - 1
        return L.MOCA_GN_ROUTE_SLAB8 if cpg % 8 == 0 else L.MOCA_GN_ROUTE_SLAB4 if cpg % 4 == 0 else L.MOCA_GN_ROUTE_SLAB2
    return L.MOCA_GN_ROUTE_STREAM


# ----------------------------------------------------------------------------------------------------------------- geometry
def chunk_geom(F, HW, C):
    """the (F, nchunk) x (C / 8, ppb) grid of the streaming, apply, concat and accum kernels; nchunk from the library"""
    nchunk = ops.groupnorm_nchunk(F, HW)
    pc = (HW + nchunk - 1) // nchunk
    return dict(nchunk=nchunk, pc=pc, ppb=max(256 // (C // 8), 1), live=(HW + pc - 1) // pc)


def chunk_bounds(HW, g):
    """[(first row, one past the last row)] of the chunks that hold rows"""
    return [(i * g["pc"], min((i + 1) * g["pc"], HW)) for i in range(g["live"])]


def rows_of_thread(n, ppb, py):
    """rows thread row `py` of a block meets in a chunk of n rows"""
    return max((n - py + ppb - 1) // ppb, 0)


def in_remainder(o, n, ppb):
    """statistics passes: is row offset o of a chunk of n rows read by the remainder loop (not by a four-row trip)?"""
    py, k = o % ppb, o // ppb
    return k >= rows_of_thread(n, ppb, py) // 4 * 4


def slab_geom(F, HW, C, fps, route):
    """what gn_plan derives for the slab kernels (restated from csrc/norm.hip; the ROUTE comes from the query)"""
    cpg, R, n_slabs = C // GROUPS, fps * HW, (F // fps) * GROUPS
    name = ROUTE_NAME[route]
    if name.startswith("slabreg"):
        vpr = cpg // 8
        nchunks = R * vpr
        cpt = (nchunks + 1023) // 1024
        return dict(R=R, vpr=vpr, nchunks=nchunks, cpt=cpt, thr=((nchunks + cpt - 1) // cpt + 63) // 64 * 64)
    S = max(min(1024 // n_slabs, 16, R), 1)
    return dict(R=R, vpr=cpg // int(name[4:]), S=S, rps=(R + S - 1) // S)


def split_bounds(sg):
    return [(s * sg["rps"], min((s + 1) * sg["rps"], sg["R"])) for s in range(sg["S"]) if s * sg["rps"] < sg["R"]]


def positions(F, HW, C, fps, route=L.MOCA_GN_ROUTE_STREAM):
    """rows (index inside a statistics group of R = fps * HW rows) where the spike goes, one after the other"""
    R = fps * HW
    P = [0, R - 1]
    if route == L.MOCA_GN_ROUTE_STREAM:
        g = chunk_geom(F, HW, C)
        b = chunk_bounds(HW, g)
        px = [0, HW - 1]
        for lo, hi in {b[0], b[-1]}:
            n, ppb = hi - lo, g["ppb"]
            px += [lo, hi - 1]
            for pred in (lambda o: not in_remainder(o, n, ppb), lambda o: in_remainder(o, n, ppb), lambda o: o // ppb >= 4,
                         lambda o: o // ppb < 4):                          # four-row trips, remainder loop, prefetched / first apply trip
                hit = [o for o in range(n) if pred(o)]
                px += [lo + hit[0], lo + hit[-1]] if hit else []
        if len(b) > 1:
            px += [b[1][0], b[-1][0] - 1]
        P += px
        if fps > 1:                                                           # the same rows in the last frame, and the frame edges
            P += [(fps - 1) * HW + p for p in px] + [HW - 1, HW]
    else:
        sg = slab_geom(F, HW, C, fps, route)
        if "S" in sg:
            sb = split_bounds(sg)
            for lo, hi in {sb[0], sb[-1], sb[len(sb) // 2]}:
                P += [lo, hi - 1]
            step = 256                                                        # pass 1 / pass 2 advance a flat vector index by 256
            P += [r for r in ((step - 1) // sg["vpr"], step // sg["vpr"], (2 * step - 1) // sg["vpr"], sb[-1][0] + step // sg["vpr"]) if r < R]
        else:
            for i in range(1, sg["cpt"] + 1):                                 # the register chunks: thread wrap and tail
                P += [r for r in ((i * sg["thr"] - 1) // sg["vpr"], (i * sg["thr"]) // sg["vpr"]) if r < R]
            P += [(sg["nchunks"] - 1) // sg["vpr"], (sg["thr"] * (sg["cpt"] - 1)) // sg["vpr"]]
        if fps > 1:
            P += [HW - 1, HW, (fps - 1) * HW]
    return sorted({p for p in P if 0 <= p < R})


# ----------------------------------------------------------------------------------------------------------------- cases
def _gn(F, HW, C, fps, route, knob=1, silu=True):
    return dict(entry="groupnorm", name="gn_%s_k%d_%dx%dx%d_fps%d" % (route, knob, F, HW, C, fps), F=F, HW=HW, C=C, fps=fps, knob=knob,
                route=route, silu=silu)


GN_CASES = [
    # default knob.  slab<2>: vpr = 5 and R % S != 0; S clamped to R = 3; cpg 30 with per-video statistics
    _gn(4, 100, 320, 1, "slab2"), _gn(1, 3, 64, 1, "slab2", silu=False), _gn(8, 64, 960, 8, "slab2"),
    # slab<4> (cpg 20: the 640-channel level): per frame; per video; rps = 3, the last splits empty; vpr = 1 (cpg 4); vpr = 3 (cpg 12)
    _gn(8, 64, 640, 1, "slab4"), _gn(8, 256, 640, 8, "slab4", silu=False), _gn(2, 37, 640, 1, "slab4"), _gn(2, 50, 128, 1, "slab4"),
    _gn(2, 50, 384, 1, "slab4", silu=False),
    # slab<8>: fewer than 256 chunks; more than 4096; cpg = 128 (the s_sc[128] / tid < cpg limit); two frames per group
    _gn(1, 8, 1280, 1, "slab8"), _gn(1, 1024, 1280, 1, "slab8", silu=False), _gn(1, 8, 4096, 1, "slab8"), _gn(4, 13, 1280, 2, "slab8"),
    # register slab, cpg 40: 260 / 1025 / 2050 / 3075 / 4095 chunks -> 1, 2, 3, 4, 4 per thread, tail threads; 4100 leaves for slab<8>
    _gn(2, 52, 1280, 1, "slabreg1"), _gn(2, 205, 1280, 1, "slabreg2", silu=False), _gn(2, 410, 1280, 1, "slabreg3"),
    _gn(2, 615, 1280, 1, "slabreg4"), _gn(2, 819, 1280, 1, "slabreg4", silu=False), _gn(2, 820, 1280, 1, "slab8"),
    # cpg 8: 256 and 4096 chunks stay, 255 leaves; cpg 128: 16 rows = 256 chunks
    _gn(2, 256, 256, 1, "slabreg1"), _gn(1, 4096, 256, 1, "slabreg4"), _gn(2, 255, 256, 1, "slab8"), _gn(1, 16, 4096, 1, "slabreg1"),
    _gn(2, 128, 256, 2, "slabreg1"),
    # the plans' per-video forms: cpg 40 at 52 / 210 / 640 rows per group, cpg 10
    _gn(4, 26, 1280, 2, "slabreg1"), _gn(4, 105, 1280, 2, "slabreg2", silu=False), _gn(16, 40, 1280, 16, "slabreg4"), _gn(4, 100, 320, 2, "slab2"),
    # streaming by the rule: odd cpg (3, 1), cpg 136 > 128 (544 threads; must not take a slab kernel)
    _gn(4, 57, 96, 1, "stream"), _gn(4, 100, 32, 2, "stream"), _gn(2, 9, 4352, 1, "stream"),
    # streaming forced (knob 0).  ppb 1 (C = 2048): one chunk of 2 / 4 / 7 rows; 13 chunks of 8, the last of 4
    _gn(4, 2, 2048, 1, "stream", 0), _gn(4, 4, 2048, 1, "stream", 0, False), _gn(4, 7, 2048, 1, "stream", 0), _gn(4, 100, 2048, 2, "stream", 0),
    # ppb 3 (C = 640): last chunk of 4 rows; last chunk of ONE row (57 = 7 x 8 + 1)
    _gn(4, 100, 640, 1, "stream", 0), _gn(2, 57, 640, 2, "stream", 0, False),
    # ppb 6 (C = 320)
    _gn(4, 57, 320, 1, "stream", 0), _gn(4, 100, 320, 2, "stream", 0),
    # ppb 1 (C = 1280): the plans' streaming launches of the 1280-channel levels (tensors past the slab rule)
    _gn(4, 100, 1280, 1, "stream", 0), _gn(4, 57, 1280, 2, "stream", 0, False),
    # ppb 64 (C = 32): 512 chunks of 9 rows, empty from chunk 456 on; finalize over 2048 and over 2040 partials
    _gn(4, 4097, 32, 1, "stream", 0), _gn(16, 1024, 32, 16, "stream", 0), _gn(12, 1360, 32, 12, "stream", 0, False),
]

CHUNK_CS = (64, 320, 640, 1280, 2560)
GSTAT_EXTRA_CS = (960, 1920)                  # cpg 30 and 60: the GroupNorm of a materialised 640 + 320 / 1280 + 640 concat
CHUNK_SHAPES = ((4, 100), (4, 5))             # 13 chunks of 8 rows, the last of 4; one chunk of 5


def _chunk_cases():
    out = []
    for C in CHUNK_CS:
        for n, (F, HW) in enumerate(CHUNK_SHAPES):
            fps = (1, 2)[(C // 64 + n) % 2]
            for entry in ("gstat", "colsum"):
                out.append(dict(entry=entry, name="%s_%dx%dx%d_fps%d" % (entry, F, HW, C, fps), F=F, HW=HW, C=C, fps=fps, silu=entry == "gstat"))
    for C in GSTAT_EXTRA_CS:
        out.append(dict(entry="gstat", name="gstat_4x100x%d_fps1" % C, F=4, HW=100, C=C, fps=1, silu=True))
    return out


CAT_PAIRS = ((320, 320), (640, 320), (640, 640), (1280, 640), (1280, 1280))


def _cat_cases():
    out = []
    for C1, C2 in CAT_PAIRS:
        for mode in ("none", "b", "fb"):
            for fps in (1, 2):
                out.append(dict(entry="cat", name="cat_%s_4x100x%d+%d_fps%d" % (mode, C1, C2, fps), F=4, HW=100, C1=C1, C2=C2, C=C1 + C2, fps=fps,
                                mode=mode, Fb=2 if mode == "fb" else 4, silu=mode != "b"))
        out.append(dict(entry="cat", name="cat_b_4x5x%d+%d_fps1" % (C1, C2), F=4, HW=5, C1=C1, C2=C2, C=C1 + C2, fps=1, mode="b", Fb=4, silu=True))
        for n, (F, HW) in enumerate(CHUNK_SHAPES):
            out.append(dict(entry="concat", name="concat_%dx%dx%d+%d_fps%d" % (F, HW, C1, C2, 1 + n), F=F, HW=HW, C1=C1, C2=C2, C=C1 + C2, fps=1 + n,
                            silu=True))
    return out


ACCUM_GROUPINGS = ((320, 20, 0), (320, 20, 320), (320, 30, 640), (640, 30, 0), (640, 40, 640), (640, 60, 1280), (1280, 60, 0), (1280, 80, 1280),
                   (8, 1, 3), (1280, 80, 0))


def _accum_cases():
    """the source is channels [coff, coff + Cn) of a tensor of C = 32 cpg channels; the test writes the rest's share itself"""
    out = []
    for n, (Cn, cpg, coff) in enumerate(ACCUM_GROUPINGS):
        for m, (F, HW) in enumerate(CHUNK_SHAPES):
            fps = (1, 2)[(n + m) % 2]
            out.append(dict(entry="accum", name="accum_%dx%dx%d_cpg%d_coff%d_fps%d" % (F, HW, Cn, cpg, coff, fps), F=F, HW=HW, Cn=Cn, cpg=cpg, coff=coff,
                            C=GROUPS * cpg, fps=fps, silu=False))
    return out


CASES = {c["name"]: c for c in GN_CASES + _chunk_cases() + _cat_cases() + _accum_cases()}
assert len(CASES) == len(GN_CASES) + len(_chunk_cases()) + len(_cat_cases()) + len(_accum_cases())


def case_route(c):
    """the route of a case as the library answers it now (the caller has set the case's knob)"""
    return ops.groupnorm_route(c["F"], c["HW"], c["C"], c["fps"]) if c["entry"] == "groupnorm" else L.MOCA_GN_ROUTE_STREAM


def case_positions(c):
    """spike rows of a case.  The chunked entries share the streaming geometry; a two-source or accum kernel's block spans ITS channels"""
    if c["entry"] == "groupnorm":
        return positions(c["F"], c["HW"], c["C"], c["fps"], case_route(c))
    return positions(c["F"], c["HW"], c.get("Cn", c["C"]), c["fps"])


def n_rounds(c):
    n_sg = c["F"] // c["fps"]
    if c["entry"] == "cat" and c["mode"] == "fb":
        n_sg = c["Fb"] // c["fps"]                    # b repeats after Fb frames: its spikes do too
    return -(-len(case_positions(c)) // n_sg)


# ----------------------------------------------------------------------------------------------------------------- inputs
SG_SCALE = (1.0, 1.5, 0.75, 1.25)     # the spike of statistics group sg: its statistics differ from its neighbours' by a factor


def group_pattern(C, cpg):
    """per channel of a C-channel tensor grouped by cpg: (offset of the noise, spike value)"""
    g = torch.arange(C) // cpg
    off = 0.1 * ((g % 4).double() - 1.5)
    amp = torch.tensor([6.0, 8.0, 10.0], dtype=torch.float64)[g % 3] * (1.0 - 2.0 * (g % 2).double())
    return off, amp


def spike_input(c, rnd):
    """fp16 [F][HW][C] (the whole normalised tensor of the case), f32 gamma, beta [C]"""
    F, HW, C, fps = c["F"], c["HW"], c["C"], c["fps"]
    g = gen(seed_of(c["name"]) + rnd)
    off, amp = group_pattern(C, C // GROUPS)
    x = 0.05 * torch.randn(F, HW, C, generator=g, dtype=torch.float64) + off
    P, n_sg = case_positions(c), F // fps
    xs = x.view(n_sg, fps * HW, C)
    for sg in range(n_sg):
        xs[sg, P[(rnd * n_sg + sg) % len(P)]] += amp * SG_SCALE[sg % 4]
    if c["entry"] == "cat" and c["mode"] == "fb":     # b = F / Fb copies of its first Fb frames; a's spikes differ between the copies
        x[:, :, c["C1"]:] = x[:c["Fb"], :, c["C1"]:].repeat(F // c["Fb"], 1, 1)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    return x.half(), gamma, beta


def plain_input(c):
    """no spike: noise of std 0.5 around the group offsets -- every row of a block weighs the same in the per-block metric"""
    F, HW, C = c["F"], c["HW"], c["C"]
    g = gen(seed_of(c["name"]) + 1000)
    x = 0.5 * torch.randn(F, HW, C, generator=g, dtype=torch.float64) + group_pattern(C, C // GROUPS)[0]
    if c["entry"] == "cat" and c["mode"] == "fb":
        x[:, :, c["C1"]:] = x[:c["Fb"], :, c["C1"]:].repeat(F // c["Fb"], 1, 1)
    return x.half(), 1.0 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


def grid_input(F, HW, C, seed):
    """multiples of 1/8 in [-4, 4]"""
    return (torch.randint(-32, 33, (F, HW, C), generator=gen(seed)).double() / 8).half()


def grid_exact(c):
    """fp32 partials of the accumulating kernels stay exact: a block's partial covers pc rows x cpg channels of squares <= 1024 units"""
    g = chunk_geom(c["F"], c["HW"], c.get("Cn", c["C"]))
    return g["pc"] * c.get("cpg", c["C"] // GROUPS) * 16 * 64 < (1 << 24)


# ----------------------------------------------------------------------------------------------------------------- reference
def reference(x, gamma, beta, fps, eps=EPS, silu=False):
    """two-pass float64 GroupNorm(32) (+SiLU) of x [F][HW][C]"""
    F, HW, C = x.shape
    xd = x.double().view(F // fps, fps * HW, GROUPS, C // GROUPS)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = (xd - mean).pow(2).mean(dim=(1, 3), keepdim=True)
    y = ((xd - mean) / torch.sqrt(var + eps)).view(F, HW, C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def stats_sums(x, fps, cpg, coff=0, w=None, n_sg=None):
    """x [F][HW][Cn] -> float64 (sum, sum of squares) [n_sg][32]: frame f counts for statistics group f // fps, channel c for group
    (coff + c) // cpg, row weights w [F][HW] (1); what falls outside [n_sg] x [32] is dropped"""
    F, HW, Cn = x.shape
    xd = x.double()
    n_sg = n_sg or F // fps
    ws = xd if w is None else xd * w[..., None]
    cs, cq = ws.sum(1), (ws * xd).sum(1)
    A = (torch.arange(F)[None] // fps == torch.arange(n_sg)[:, None]).double()
    B = ((coff + torch.arange(Cn))[:, None] // cpg == torch.arange(GROUPS)[None]).double()
    return A @ cs @ B, A @ cq @ B


def to_fixed(S, Q):
    """the i64 accumulators [n_sg][32][2] holding these sums"""
    return torch.stack([torch.round(S * SUM_SCALE), torch.round(Q * SQ_SCALE)], -1).to(torch.int64)


def from_fixed(acc):
    a = acc.double()
    return a[..., 0] / SUM_SCALE, a[..., 1] / SQ_SCALE


def finish(S, Q, count, eps=EPS):
    mean = S / count
    return mean, 1.0 / torch.sqrt((Q / count - mean * mean).clamp_min(0.0) + eps)


def apply_norm(x, mean, rstd, gamma, beta, fps, cpg, silu):
    """y = (x - mean) rstd gamma + beta with frame f reading statistics group f // fps, channel c group c // cpg (clamped into the table)"""
    F, HW, C = x.shape
    si = (torch.arange(F) // fps).clamp(max=mean.shape[0] - 1)
    gi = (torch.arange(C) // cpg).clamp(max=GROUPS - 1)
    m, r = mean[si][:, gi][:, None], rstd[si][:, gi][:, None]
    y = (x.double() - m) * r * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def merge_b(Sa, Sb, C1, C2, sgb_mod, wrong=None):
    """gn_apply_gstat_cat_kernel's merge of b's own groups (C2 / 32 channels each) into the concat's: [n_sg][32] (+)= [n_sgb][32]"""
    cpg, cpg2 = (C1 + C2) // GROUPS, C2 // GROUPS
    out = Sa.clone()
    for sg in range(Sa.shape[0]):
        sb = sg if wrong == "fb_ignored" else sg % sgb_mod
        for t in range(GROUPS):
            tt = t + 1 if wrong == "b_group_to_neighbour" else t
            lo, hi = max(tt * cpg - C1, 0), min((tt + 1) * cpg - C1, C2)
            j = lo // cpg2
            while j * cpg2 < hi:
                if sb < Sb.shape[0] and j < GROUPS:
                    out[sg, t] += Sb[sb, j]
                j += 1
    return out


# ----------------------------------------------------------------------------------------------------------------- wrong restatements
MUTATIONS = ("drop_chunk_last_row", "drop_remainder_rows", "chunk_first_row_twice", "cpg_plus_1", "cpg_minus_1", "fps_plus_1", "fps_minus_1",
             "coff_ignored", "fb_ignored", "b_group_to_neighbour", "split_off_by_one", "slab_drops_last_row", "silu_dropped")
_ROW = ("drop_chunk_last_row", "drop_remainder_rows", "chunk_first_row_twice")


def row_weights(F, HW, C, wrong):
    """[F][HW] multiplicity of every row under a wrong chunk walk of the (F, nchunk) x (C / 8, ppb) grid"""
    g = chunk_geom(F, HW, C)
    w = torch.ones(HW, dtype=torch.float64)
    for lo, hi in chunk_bounds(HW, g):
        if wrong == "drop_chunk_last_row":
            w[hi - 1] = 0
        elif wrong == "chunk_first_row_twice":
            w[lo] = 2
        elif wrong == "drop_remainder_rows":
            for o in range(hi - lo):
                if in_remainder(o, hi - lo, g["ppb"]):
                    w[lo + o] = 0
    return w[None].expand(F, HW)


def mutations_of(c):
    """the wrong restatements that change what this case computes"""
    e, F, fps = c["entry"], c["F"], c["fps"]
    route = case_route(c)
    m = []
    if route == L.MOCA_GN_ROUTE_STREAM:
        wc = c.get("Cn", c["C"])
        rows = [x for x in _ROW if not torch.equal(row_weights(1, c["HW"], wc, x), torch.ones(1, c["HW"], dtype=torch.float64))]
        m += [x for x in rows if x != "chunk_first_row_twice" or e in ("groupnorm", "concat", "accum")]   # (an apply pass has no "twice")
    else:
        m += ["slab_drops_last_row"] + (["split_off_by_one"] if "S" in slab_geom(F, c["HW"], c["C"], fps, route) else [])
    cpg = c.get("cpg", c["C"] // GROUPS)
    m += ["cpg_plus_1"] + (["cpg_minus_1"] if cpg > 1 else [])
    m += (["fps_plus_1"] if F > fps else []) + (["fps_minus_1"] if fps > 1 else [])       # (one statistics group: f // (fps + 1) is f // fps)
    if e == "accum" and c["coff"]:
        m.append("coff_ignored")
    if e == "cat" and c["mode"] == "fb":
        m.append("fb_ignored")
    if e == "cat" and c["mode"] in ("b", "fb"):
        m.append("b_group_to_neighbour")
    if c["silu"]:
        m.append("silu_dropped")
    return m


def restated(c, inp, wrong=None):
    """float64 output [F][HW][C] of the case's launch sequence restated from sums, with one wrong restatement.  The statistics the TEST
    writes (gstat, colsum, gstat_cat, gstat_b, the rest's share of an accum case) are always right: the mutation sits in the kernel."""
    x, gamma, beta = inp
    e, F, HW, C, fps = c["entry"], c["F"], c["HW"], c["C"], c["fps"]
    cpg, n_sg = C // GROUPS, F // fps
    count = fps * HW * cpg
    cpg_w = cpg + 1 if wrong == "cpg_plus_1" else cpg - 1 if wrong == "cpg_minus_1" else cpg
    fps_w = fps + 1 if wrong == "fps_plus_1" else fps - 1 if wrong == "fps_minus_1" else fps
    silu = c["silu"] and wrong != "silu_dropped"
    route = case_route(c)
    stream = route == L.MOCA_GN_ROUTE_STREAM
    produces = e in ("groupnorm", "concat", "accum")          # the kernel under test makes statistics (else it only applies them)
    w = row_weights(F, HW, c.get("Cn", C), wrong) if wrong in _ROW and stream else None
    if wrong == "slab_drops_last_row":
        w = torch.ones(n_sg, fps * HW, dtype=torch.float64)
        w[:, -1] = 0
        w = w.view(F, HW)
    if e == "accum":
        Cn, coff, gw = c["Cn"], c["coff"], c["cpg"]
        S, Q = torch.zeros(n_sg, GROUPS, dtype=torch.float64), torch.zeros(n_sg, GROUPS, dtype=torch.float64)
        for lo, hi in ((0, coff), (coff + Cn, C)):            # the rest's share, written by the test
            if hi > lo:
                s_, q_ = stats_sums(x[:, :, lo:hi], fps, gw, lo)
                S, Q = S + s_, Q + q_
        gw_w = gw + 1 if wrong == "cpg_plus_1" else gw - 1 if wrong == "cpg_minus_1" else gw
        S1, Q1 = stats_sums(x[:, :, coff:coff + Cn], fps_w, gw_w, 0 if wrong == "coff_ignored" else coff, w, n_sg)
        mean, rstd = finish(S + S1, Q + Q1, count)
        return apply_norm(x, mean, rstd, gamma, beta, fps, cpg, silu)      # (the apply is groupnorm_gstat, not under test here)
    if produces:
        S, Q = stats_sums(x, fps_w, cpg_w, 0, w, n_sg)
    else:
        S, Q = stats_sums(x, fps, cpg)
        if e == "cat" and c["mode"] != "none":
            C1, C2 = c["C1"], c["C2"]
            Sa, Qa = stats_sums(x[:, :, :C1], fps, cpg)
            Sb, Qb = stats_sums(x[:c["Fb"], :, C1:], fps, C2 // GROUPS)
            S, Q = merge_b(Sa, Sb, C1, C2, c["Fb"] // fps, wrong), merge_b(Qa, Qb, C1, C2, c["Fb"] // fps, wrong)
    mean, rstd = finish(S, Q, count)
    if e == "concat":                                          # (the apply is groupnorm_gstat, not under test here)
        return apply_norm(x, mean, rstd, gamma, beta, fps, cpg, silu)
    y = apply_norm(x, mean, rstd, gamma, beta, fps_w, cpg_w, silu)
    if w is not None and not produces:                         # an apply pass that skips rows leaves them unwritten
        y = torch.where((w > 0)[..., None], y, torch.full_like(y, SENTINEL))
    if wrong == "split_off_by_one":
        yv = y.view(n_sg, fps * HW, C)
        for lo, hi in split_bounds(slab_geom(F, HW, C, fps, route)):
            yv[:, hi - 1] = SENTINEL
    return y


# ----------------------------------------------------------------------------------------------------------------- metric
def block_errors(got, ref, fps):
    """max|got - ref| / max|ref| per (statistics group, channel group) block of [F][HW][C] tensors -> [n_sg][32]"""
    F, HW, C = ref.shape
    g = got.double().cpu().view(F // fps, fps * HW, GROUPS, C // GROUPS)
    r = ref.double().cpu().view(F // fps, fps * HW, GROUPS, C // GROUPS)
    d = torch.nan_to_num((g - r).abs(), nan=float("inf")).amax(dim=(1, 3))
    return d / r.abs().amax(dim=(1, 3)).clamp_min(1e-30)


WORST = {}                      # route / entry -> worst block error seen (printed by the GPU tests)


def check_blocks(got, ref, fps, what, group=None, tol=TOL16):
    e = block_errors(got, ref, fps)
    worst = e.max().item()
    if group is not None:
        WORST[group] = max(WORST.get(group, 0.0), worst)
    bad = (e > tol).nonzero().tolist()
    assert not bad, f"{what}: {len(bad)} (statistics group, channel group) blocks beyond {tol:.1e}, first {bad[:4]}, worst {worst:.2e}"
    return worst


# ----------------------------------------------------------------------------------------------------------------- launches (GPU)
DEV = "cuda"
GUARD = 4                       # guard rows in front of and behind every operand
NAN = float("nan")
POISON = 1 << 62                # an accumulator that reads as NaN (csrc/common.h)


class Guarded:
    """a contiguous tensor of `shape` with GUARD rows of `fill` in front of it and behind it (a row = the last dimension)"""

    def __init__(self, shape, dtype, fill, data=None, inner=None):
        shape = tuple(shape)
        self.row = shape[-1]
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD * self.row,), fill, dtype=dtype, device=DEV)
        self.fill = fill
        self.t = self.buf[GUARD * self.row:GUARD * self.row + n].view(shape)
        if data is not None:
            self.t.copy_(data.to(DEV).to(dtype))
        elif inner is not None:
            self.t.fill_(inner)

    def assert_guards(self, what):
        g = torch.cat([self.buf[:GUARD * self.row], self.buf[self.buf.numel() - GUARD * self.row:]])
        ok = torch.isnan(g).all() if self.fill != self.fill else (g == self.fill).all()
        assert ok, f"{what}: a store landed outside the operand"


def gin(data, dtype=None):
    """an input: guards that read as NaN (fp16 / f32) or as a poisoned accumulator (i64)"""
    dtype = dtype or data.dtype
    return Guarded(data.shape, dtype, POISON if dtype == torch.int64 else NAN, data=data)


def gout(shape, dtype=torch.float16):
    return Guarded(shape, dtype, SENTINEL, inner=SENTINEL)


def fixed(S, Q):
    return gin(to_fixed(S, Q))


def run_case(c, inp):
    """the launches of one case on guarded operands -> (y [F][HW][C] on the host, what to check afterwards)"""
    x, gamma, beta = inp
    e, F, HW, Cn, fps = c["entry"], c["F"], c["HW"], c["C"], c["fps"]
    cpg = Cn // GROUPS
    gx, gg, gb, gy = gin(x), gin(gamma), gin(beta), gout((F, HW, Cn))
    held = [gx, gg, gb, gy]
    kw = dict(F=F, HW=HW, frames_per_stat=fps, eps=EPS, silu=c["silu"])
    if e == "groupnorm":
        assert ROUTE_NAME.get(ops.groupnorm_route(F, HW, Cn, fps)) == c["route"], c["name"]
        ws = Guarded((ops.groupnorm_ws_floats(F, HW, Cn),), torch.float32, 12345.0, inner=0.0)
        held.append(ws)
        ops.groupnorm(gx.t, gy.t, gg.t, gb.t, Cn=Cn, ws=ws.t, **kw)
    elif e == "gstat":
        gs = fixed(*stats_sums(x, fps, cpg))
        held.append(gs)
        ops.groupnorm_gstat(gx.t, gy.t, gg.t, gb.t, gs.t, Cn=Cn, **kw)
    elif e == "colsum":
        tile = HW // 5 if HW % 5 == 0 and HW > 5 else HW
        xd = x.double().view(F * HW // tile, tile, Cn)
        cs = gin(torch.stack([xd.sum(1), (xd * xd).sum(1)], -1).float())          # fp32 column sums [row tile][C][2]
        ws = Guarded((ops.groupnorm_ws_floats(F, HW, Cn),), torch.float32, 12345.0, inner=0.0)
        held += [cs, ws]
        ops.groupnorm_colsum(gx.t, gy.t, gg.t, gb.t, cs.t, tile_rows=tile, Cn=Cn, ws=ws.t, **kw)
    elif e == "cat":
        C1, C2 = c["C1"], c["C2"]
        ga, gbb = gin(x[:, :, :C1].contiguous()), gin(x[:, :, C1:].contiguous())
        if c["mode"] == "none":
            gcat, gsb = fixed(*stats_sums(x, fps, cpg)), None
        else:
            gcat = fixed(*stats_sums(x[:, :, :C1], fps, cpg))                    # a's share, in the concat's grouping
            gsb = fixed(*stats_sums(x[:c["Fb"], :, C1:], fps, C2 // GROUPS))     # b's own statistics of its Fb frames
            held.append(gsb)
        held += [ga, gbb, gcat]
        ops.groupnorm_gstat_cat(ga.t, gbb.t, gy.t, gg.t, gb.t, gcat.t, gsb.t if gsb else None, C1=C1, C2=C2, Fb=c["Fb"] if c["mode"] == "fb" else 0, **kw)
    elif e == "concat":
        C1, C2 = c["C1"], c["C2"]
        ga, gbb, gcat_out = gin(x[:, :, :C1].contiguous()), gin(x[:, :, C1:].contiguous()), gout((F, HW, Cn))
        gs = Guarded((F // fps, GROUPS, 2), torch.int64, POISON, inner=0)
        held += [ga, gbb, gcat_out, gs]
        ops.concat_channels_gstat(ga.t, gbb.t, gcat_out.t, gs.t, F=F, HW=HW, C1=C1, C2=C2, frames_per_stat=fps)
        assert torch.equal(gcat_out.t.cpu(), x), f"{c['name']}: the concat is not its sources"
        ops.groupnorm_gstat(gcat_out.t, gy.t, gg.t, gb.t, gs.t, Cn=Cn, **kw)
    else:
        Cs, gw, coff = c["Cn"], c["cpg"], c["coff"]
        S, Q = torch.zeros(F // fps, GROUPS, dtype=torch.float64), torch.zeros(F // fps, GROUPS, dtype=torch.float64)
        for lo, hi in ((0, coff), (coff + Cs, Cn)):                                # the rest of the tensor: its share is written here
            if hi > lo:
                s_, q_ = stats_sums(x[:, :, lo:hi], fps, gw, lo)
                S, Q = S + s_, Q + q_
        gsrc, gs = gin(x[:, :, coff:coff + Cs].contiguous()), fixed(S, Q)
        held += [gsrc, gs]
        ops.gstat_accum(gsrc.t, gs.t, F=F, HW=HW, Cn=Cs, frames_per_stat=fps, cpg=gw, coff=coff)
        ops.groupnorm_gstat(gx.t, gy.t, gg.t, gb.t, gs.t, Cn=Cn, **kw)
    torch.cuda.synchronize()
    return gy.t.cpu(), held


def accum_start(n_sg):
    """accumulators [n_sg][32][2] that are not zero before a launch adds to them: sums of either sign, sums of squares >= 0"""
    idx = torch.arange(n_sg * GROUPS, dtype=torch.int64).view(n_sg, GROUPS)
    return torch.stack([idx * 7919 - 100000, idx * 104729 + 1], -1)


def accumulate(c, x, start):
    """the concat / accum launch of a case alone, on its input x ([F][HW][C1 + C2] / the source [F][HW][Cn]) and accumulators that hold
    `start` -> (the accumulators, the concat's output or None, the guarded accumulators and output)"""
    F, HW, fps = c["F"], c["HW"], c["fps"]
    gs = gin(start)
    if c["entry"] == "concat":
        C1, C2 = c["C1"], c["C2"]
        ga, gb, go = gin(x[:, :, :C1].contiguous()), gin(x[:, :, C1:].contiguous()), gout((F, HW, C1 + C2))
        ops.concat_channels_gstat(ga.t, gb.t, go.t, gs.t, F=F, HW=HW, C1=C1, C2=C2, frames_per_stat=fps)
    else:
        gx, go = gin(x), None
        ops.gstat_accum(gx.t, gs.t, F=F, HW=HW, Cn=c["Cn"], frames_per_stat=fps, cpg=c["cpg"], coff=c["coff"])
    torch.cuda.synchronize()
    return gs.t.cpu(), go.t.cpu() if go else None, [gs] + ([go] if go else [])


# ----------------------------------------------------------------------------------------------------------------- fold weights
def fold_weights(w, gamma, S, Q, count, eps, K):
    """moca_groupnorm_fold_weights_f16 in float64 on w [N][ldw] (fp16), statistics (S, Q) [n_sg][32]: wg as the kernel's fp32 product
    rounded to fp16 would be, exactly (wg_exact), and bg from the STORED wg handed in by the caller (see fold_bias)"""
    mean, rstd = finish(S, Q, count, eps)
    gi = torch.arange(K) // (K // GROUPS)
    s = rstd[:, gi] * gamma.double()[None]                    # [n_sg][K]
    return w.double()[None, :, :K] * s[:, None, :], mean[:, gi]


def fold_bias(w, bias, beta, wg_stored, mean_k, K):
    """bg [n_sg][N] = bias + sum_k beta_k w[n][k] - sum_k mean_g(k) wg[sg][n][k], and sum of |terms| of every row (the fp32 summation bound)"""
    wd, wgd = w.double()[:, :K], wg_stored.double()[:, :, :K]
    t1 = wd * beta.double()[None]                             # [N][K]
    t2 = mean_k[:, None, :] * wgd                             # [n_sg][N][K]
    b = bias.double()[None] if bias is not None else 0.0
    bg = b + t1.sum(1)[None] - t2.sum(2)
    mag = (bias.double().abs()[None] if bias is not None else 0.0) + t1.abs().sum(1)[None] + t2.abs().sum(2)
    return bg, mag


def fold_operands(K, bias):
    """host operands of one moca_groupnorm_fold_weights_f16 case: N = 72 (four whole 16-row blocks and one of 8), ldw = K + 8 (zero pad
    columns), n_sg = 3, the statistics as accumulators `acc`"""
    N, ldw, n_sg, eps = 72, K + 8, 3, 1e-6
    count = 640 * (K // GROUPS)
    g = gen(500 + K + bias)
    w = torch.zeros(N, ldw, dtype=torch.float16)
    w[:, :K] = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    bi = torch.randn(N, generator=g) if bias else None
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    mean = 3.0 * torch.randn(n_sg, GROUPS, generator=g, dtype=torch.float64)
    var = 0.25 + torch.rand(n_sg, GROUPS, generator=g, dtype=torch.float64) * 4
    acc = to_fixed(mean * count, (var + mean * mean) * count)
    return dict(K=K, N=N, ldw=ldw, n_sg=n_sg, eps=eps, count=count, w=w, bias=bi, gamma=gamma, beta=beta, acc=acc)


def fold_run(o):
    """the launch on guarded operands -> (wg [n_sg][N][ldw], bg [n_sg][N] on the host, the guarded operands)"""
    N, ldw, n_sg = o["N"], o["ldw"], o["n_sg"]
    gw, gbi, gg, gb, gs = gin(o["w"]), gin(o["bias"]) if o["bias"] is not None else None, gin(o["gamma"]), gin(o["beta"]), gin(o["acc"])
    gwg, gbg = gout((n_sg * N, ldw)), gout((n_sg * N,), torch.float32)
    rc = L.load().moca_groupnorm_fold_weights_f16(L.ptr(gw.t), L.ptr(gbi.t) if gbi else None, L.ptr(gg.t), L.ptr(gb.t), L.ptr(gs.t), L.ptr(gwg.t),
                                                  L.ptr(gbg.t), n_sg, N, o["K"], ldw, o["count"], o["eps"], None)
    assert rc == 0
    torch.cuda.synchronize()
    return gwg.t.cpu().view(n_sg, N, ldw), gbg.t.cpu().view(n_sg, N), [gw, gg, gb, gs, gwg, gbg] + ([gbi] if gbi else [])


# ----------------------------------------------------------------------------------------------------------------- census
def gn_class(F, HW, C, fps):
    """class of a standalone GroupNorm launch: (route name, channels per group, statistics over several frames?)"""
    return (ROUTE_NAME.get(ops.groupnorm_route(F, HW, C, fps), "refused"), C // GROUPS, fps > 1)


def launch_class(name, args, kw):
    """class of one norm-family launch of a plan (a functools.partial's func name, args, keywords), None for any other launch"""
    if name == "groupnorm":
        return ("groupnorm",) + gn_class(kw["F"], kw["HW"], kw["Cn"], kw["frames_per_stat"])
    if name in ("groupnorm_gstat", "groupnorm_colsum"):
        return (name[10:], kw["Cn"] // GROUPS, kw["frames_per_stat"] > 1)
    if name == "concat_channels_gstat":
        return ("concat", kw["C1"], kw["C2"], kw["frames_per_stat"] > 1)
    if name == "gstat_accum":
        return ("accum", kw["Cn"], kw["cpg"], kw["coff"] % kw["cpg"] != 0, kw["coff"] > 0, kw["frames_per_stat"] > 1)
    if name == "groupnorm_gstat_cat":
        Fb = kw.get("Fb") or kw["F"]
        return ("cat", kw["C1"], kw["C2"], "gstat_b" if args[6] is not None else None, Fb < kw["F"], kw["frames_per_stat"] > 1)
    return None


def table_classes():
    """the classes the GPU table runs.  A standalone GroupNorm case counts under the route it names, however the knob got it there: the
    streaming kernels a plan reaches by tensor size are the ones MOCA_TUNE_GN_SLAB = 0 runs on the table's small tensors"""
    out = set()
    for c in CASES.values():
        e = c["entry"]
        if e == "groupnorm":
            out.add(("groupnorm", c["route"], c["C"] // GROUPS, c["fps"] > 1))
        elif e in ("gstat", "colsum"):
            out.add((e, c["C"] // GROUPS, c["fps"] > 1))
        elif e == "concat":
            out.add(("concat", c["C1"], c["C2"], c["fps"] > 1))
        elif e == "accum":
            out.add(("accum", c["Cn"], c["cpg"], c["coff"] % c["cpg"] != 0, c["coff"] > 0, c["fps"] > 1))
        elif c["mode"] != "none":
            out.add(("cat", c["C1"], c["C2"], "gstat_b", c["Fb"] < c["F"], c["fps"] > 1))
        if e == "cat" and c["mode"] == "none":
            out.add(("cat", c["C1"], c["C2"], None, False, c["fps"] > 1))
    return out


# ----------------------------------------------------------------------------------------------------------------- the parent commit's bits
# tests/test_norm_parent_gpu.py and tools/record_parent_fixtures.py --norm-sha: sha256 of what the launches leave, on host-generated
# operands.  Outputs start as the sentinel and the accumulators of the concat / accum launches start non-zero, so an element that was
# not written, or an accumulator that was overwritten instead of added to, changes the hash.
FOLD_CASES = ((320, True), (320, False), (2560, True))
BIG = (16, 65536, 64)           # 128 MiB of fp16 exactly: the smallest tensor that leaves with non-temporal stores
PARENT_GROUPS = ("groupnorm", "gstat", "colsum", "cat", "concat", "accum", "fold", "big")


def sha(*tensors):
    import hashlib
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def parent_names(group):
    if group == "fold":
        return ["fold_%d_bias%d" % (K, b) for K, b in FOLD_CASES]
    if group == "big":
        return ["big_%dx%dx%d.%s" % (BIG + (k,)) for k in ("concat", "gstat", "cat")]
    return [n + "." + k for n, c in CASES.items() if c["entry"] == group for k in ("plain", "spike")]


def _big_hashes():
    """the BIG shape through concat_channels_gstat, groupnorm_gstat and groupnorm_gstat_cat (a grid tensor: the concat's accumulators are
    exact, whatever order its blocks arrive in)"""
    F, HW, Cn = BIG
    C1 = C2 = Cn // 2
    g = gen(77)
    x = (torch.randint(-32, 33, (F, HW, Cn), generator=g, dtype=torch.int8).to(torch.float16) / 8).to(DEV)
    gamma, beta = (1.0 + 0.2 * torch.randn(Cn, generator=g)).to(DEV), (0.2 * torch.randn(Cn, generator=g)).to(DEV)
    a, b = x[:, :, :C1].contiguous(), x[:, :, C1:].contiguous()
    out = {}
    o, gs = torch.full_like(x, SENTINEL), torch.zeros(F, GROUPS, 2, dtype=torch.int64, device=DEV)
    ops.concat_channels_gstat(a, b, o, gs, F=F, HW=HW, C1=C1, C2=C2, frames_per_stat=1)
    out["concat"] = sha(o, gs)
    o.fill_(SENTINEL)
    ops.groupnorm_gstat(x, o, gamma, beta, gs, F=F, HW=HW, Cn=Cn, frames_per_stat=1, eps=EPS, silu=True)
    out["gstat"] = sha(o)
    o.fill_(SENTINEL)
    ops.groupnorm_gstat_cat(a, b, o, gamma, beta, gs, None, F=F, HW=HW, C1=C1, C2=C2, frames_per_stat=1, eps=EPS, silu=True)
    out["cat"] = sha(o)
    return {"big_%dx%dx%d.%s" % (BIG + (k,)): v for k, v in out.items()}


def parent_hashes(group):
    """{name: sha256} of the group's launches, in the order of parent_names(group)"""
    if group == "big":
        return _big_hashes()
    if group == "fold":
        return {"fold_%d_bias%d" % (K, b): sha(*fold_run(fold_operands(K, b))[:2]) for K, b in FOLD_CASES}
    out = {}
    for n, c in CASES.items():
        if c["entry"] != group:
            continue
        old = L.set_tuning(L.MOCA_TUNE_GN_SLAB, c["knob"]) if group == "groupnorm" else None
        try:
            for kind, inp in (("plain", plain_input(c)), ("spike", spike_input(c, 0))):
                left = [run_case(c, inp)[0]]
                if group in ("concat", "accum"):
                    x = inp[0] if group == "concat" else inp[0][:, :, c["coff"]:c["coff"] + c["Cn"]].contiguous()
                    acc, o, _ = accumulate(c, x, accum_start(c["F"] // c["fps"]))
                    left += [acc] + ([o] if o is not None else [])
                out[f"{n}.{kind}"] = sha(*left)
        finally:
            if old is not None:
                L.set_tuning(L.MOCA_TUNE_GN_SLAB, old)
    return out
