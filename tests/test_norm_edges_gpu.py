"""GPU half of the norm edge suite: every kernel of the GroupNorm family of csrc/norm.hip on every dispatch route, chunk tail, split
and group edge, judged per (statistics group, channel group) block against a two-pass float64 GroupNorm (tests/norm_edges_ref.py;
tests/test_norm_edges_cpu.py shows on the host that every case tells every wrong restatement from the right one).

The route of every standalone GroupNorm case is asserted through ops.groupnorm_route before its launch.  The statistics that
groupnorm_gstat, groupnorm_colsum and groupnorm_gstat_cat consume are written by the test from float64 sums, so an apply kernel is
judged alone; the accumulators that concat_channels_gstat and gstat_accum leave are read back and must equal the integer sums."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_edges_ref as R  # noqa: E402
from moca_video_amd import lib as L  # noqa: E402
from moca_video_amd import ops  # noqa: E402

DEV = R.DEV


@pytest.fixture(autouse=True)
def _stream():
    ops.set_stream(None)
    yield
    torch.cuda.synchronize()


@pytest.fixture
def tune():
    saved = []

    def set_(knob, value):
        saved.append((knob, L.set_tuning(knob, value)))
    yield set_
    for knob, old in reversed(saved):
        L.set_tuning(knob, old)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(R.WORST):
        print(f"[worst] {k}: worst (statistics group, channel group) block {R.WORST[k]:.2e} of its max|ref| (bound {R.TOL16:.1e})")


run_case = R.run_case           # the launches of a case on guarded operands (shared with the parent-commit hashes: tests/norm_edges_ref.py)


def case_group(c):
    return "groupnorm " + c["route"] if c["entry"] == "groupnorm" else c["entry"] + (" " + c["mode"] if c["entry"] == "cat" else "")


# ---------------------------------------------------------------- 1: spike probes
@pytest.mark.parametrize("name", list(R.CASES))
def test_spike_probe(name, tune):
    """every round of the case: the spike row of every statistics group at its next edge position, per-block metric"""
    c = R.CASES[name]
    if c["entry"] == "groupnorm":
        tune(L.MOCA_TUNE_GN_SLAB, c["knob"])
    worst = 0.0
    for rnd in range(R.n_rounds(c)):
        inp = R.spike_input(c, rnd)
        y, _ = run_case(c, inp)
        worst = max(worst, R.check_blocks(y, R.reference(*inp, c["fps"], silu=c["silu"]), c["fps"], f"{name} round {rnd}", group=case_group(c)))
    print(f"[parity] {name}: worst block {worst:.2e} over {R.n_rounds(c)} rounds")


# ---------------------------------------------------------------- 2: exact accumulators
@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["entry"] in ("concat", "accum")])
def test_accumulators_exact(name):
    """multiples of 1/8: the accumulators the kernel ADDS to (non-zero before the launch) end at start + the integer sums, exactly"""
    c = R.CASES[name]
    assert R.grid_exact(c)
    F, HW, fps = c["F"], c["HW"], c["fps"]
    start = R.accum_start(F // fps)
    if c["entry"] == "concat":
        x = R.grid_input(F, HW, c["C1"] + c["C2"], R.seed_of(name))
        want = start + R.to_fixed(*R.stats_sums(x, fps, (c["C1"] + c["C2"]) // R.GROUPS))
    else:
        x = R.grid_input(F, HW, c["Cn"], R.seed_of(name))
        want = start + R.to_fixed(*R.stats_sums(x, fps, c["cpg"], c["coff"]))
    got, out, held = R.accumulate(c, x, start)
    if c["entry"] == "concat":
        assert torch.equal(out, x), f"{name}: the concat is not bit-equal to its sources"
    for h in held:
        h.assert_guards(name)
    assert torch.equal(got, want), f"{name}: {(got != want).sum().item()} accumulators differ from the integer sums, first {(got != want).nonzero()[:4].tolist()}"


# ---------------------------------------------------------------- 3: surroundings
@pytest.mark.parametrize("name", list(R.CASES))
def test_surroundings(name, tune):
    """plain noise (every row counts alike in a block).  Inputs sit between NaN rows (accumulators: poisoned), outputs between sentinel
    rows and start as the sentinel: every element is written, no guard is touched, no NaN reaches the result (the apply kernels' clamped
    prefetch reads row p_end - 1, never past it)"""
    c = R.CASES[name]
    if c["entry"] == "groupnorm":
        tune(L.MOCA_TUNE_GN_SLAB, c["knob"])
    inp = R.plain_input(c)
    y, held = run_case(c, inp)
    for h in held:
        h.assert_guards(name)
    assert torch.isfinite(y.float()).all(), f"{name}: a guard value reached the output"
    assert (y != R.SENTINEL).all(), f"{name}: {(y == R.SENTINEL).sum().item()} output elements were never written"
    R.check_blocks(y, R.reference(*inp, c["fps"], silu=c["silu"]), c["fps"], name + " (plain noise)", group=case_group(c))


# ---------------------------------------------------------------- 4: the streaming-store instantiations
BIG = [(16, 65536, 64, True), (16, 65535, 64, False)]      # 128 MiB of fp16 exactly (non-temporal stores) and 16 rows below (plain stores)


def _int_sums(x):
    """exact accumulators of a grid tensor [F][HW][C] on the device, per frame: i64 [F][32][2]"""
    F, HW, Cn = x.shape
    out = torch.empty(F, R.GROUPS, 2, dtype=torch.int64, device=x.device)
    for f in range(F):
        v = (x[f].float() * 8).to(torch.int64).view(HW, R.GROUPS, Cn // R.GROUPS)
        out[f, :, 0] = v.sum(dim=(0, 2)) * (R.SUM_SCALE // 8)
        out[f, :, 1] = (v * v).sum(dim=(0, 2)) * (R.SQ_SCALE // 64)
    return out


@pytest.mark.parametrize("F,HW,Cn,streams", BIG)
def test_streaming_store_variants(F, HW, Cn, streams):
    """gn_apply_gstat_kernel, gn_apply_gstat_cat_kernel and concat_gstat_kernel with and without non-temporal stores: every frame of
    the large call is bit-equal to the same entry on that frame alone with its slice of the statistics (the apply arithmetic does not
    depend on the chunking); the concat's accumulators are exact on a grid"""
    assert ((F * HW * Cn * 2) >= (128 << 20)) == streams
    C1 = C2 = Cn // 2
    g = torch.Generator(device=DEV).manual_seed(77)
    x = (torch.randint(-32, 33, (F, HW, Cn), generator=g, device=DEV, dtype=torch.int32).float() / 8).half()
    a, b = x[:, :, :C1].contiguous(), x[:, :, C1:].contiguous()
    gamma = (1.0 + 0.2 * torch.randn(Cn, generator=g, device=DEV)).contiguous()
    beta = (0.2 * torch.randn(Cn, generator=g, device=DEV)).contiguous()
    want = _int_sums(x)
    assert R.chunk_geom(F, HW, Cn)["pc"] * (Cn // R.GROUPS) * 1024 < (1 << 24)
    # concat + statistics
    out = torch.full_like(x, R.SENTINEL)
    gs = torch.zeros(F, R.GROUPS, 2, dtype=torch.int64, device=DEV)
    ops.concat_channels_gstat(a, b, out, gs, F=F, HW=HW, C1=C1, C2=C2, frames_per_stat=1)
    assert torch.equal(out, x) and torch.equal(gs, want)
    o1, g1 = torch.empty_like(x[0]), torch.zeros(1, R.GROUPS, 2, dtype=torch.int64, device=DEV)
    for f in (0, F - 1):
        g1.zero_()
        ops.concat_channels_gstat(a[f], b[f], o1, g1, F=1, HW=HW, C1=C1, C2=C2, frames_per_stat=1)
        assert torch.equal(o1, out[f]) and torch.equal(g1[0], gs[f])
    # the two apply kernels
    y = torch.full_like(x, R.SENTINEL)
    ops.groupnorm_gstat(x, y, gamma, beta, gs, F=F, HW=HW, Cn=Cn, frames_per_stat=1, eps=R.EPS, silu=True)
    yc = torch.full_like(x, R.SENTINEL)
    ops.groupnorm_gstat_cat(a, b, yc, gamma, beta, gs, None, F=F, HW=HW, C1=C1, C2=C2, frames_per_stat=1, eps=R.EPS, silu=True)
    y1 = torch.empty_like(x[0])
    for f in range(F):
        ops.groupnorm_gstat(x[f], y1, gamma, beta, gs[f:f + 1], F=1, HW=HW, Cn=Cn, frames_per_stat=1, eps=R.EPS, silu=True)
        assert torch.equal(y1, y[f]), f"groupnorm_gstat frame {f}: the large call differs from the frame alone"
        ops.groupnorm_gstat_cat(a[f], b[f], y1, gamma, beta, gs[f:f + 1], None, F=1, HW=HW, C1=C1, C2=C2, frames_per_stat=1, eps=R.EPS, silu=True)
        assert torch.equal(y1, yc[f]), f"groupnorm_gstat_cat frame {f}: the large call differs from the frame alone"
    for f in (0, F - 1):                                    # and the frames are right
        ref = R.reference(x[f:f + 1].cpu(), gamma.cpu(), beta.cpu(), 1, silu=True)
        R.check_blocks(y[f:f + 1], ref, 1, f"groupnorm_gstat {F}x{HW}x{Cn} frame {f}", group="gstat " + ("non-temporal" if streams else "at 128 MiB - 16 rows"))


# ---------------------------------------------------------------- 5: the fold of GroupNorm into per-group weights
@pytest.mark.parametrize("K,bias", R.FOLD_CASES)
def test_fold_weights_edges(K, bias):
    """N = 72 (four whole 16-row blocks and one of 8), ldw = K + 8 (zero pad columns come back zero), n_sg = 3, statistics written here.
    wg against the float64 product within one fp16 rounding plus the three fp32 roundings in front of it (rstd, rstd gamma, w s):
    2^-11 (1 + 2^-10) relative (+ 2^-25, half an fp16 subnormal step); bg within the fp32 summation bound K 2^-24 sum|terms| of its row,
    the mean term taken from the stored wg as the kernel takes it"""
    o = R.fold_operands(K, bias)
    w, bi, gamma, beta, count, eps = o["w"], o["bias"], o["gamma"], o["beta"], o["count"], o["eps"]
    S, Q = R.from_fixed(o["acc"])
    wg, bg, held = R.fold_run(o)
    bg = bg.double()
    for h in held:
        h.assert_guards(f"fold_weights K={K}")
    assert (wg[:, :, K:] == 0).all(), "pad columns of wg are not zero"
    exact, mean_k = R.fold_weights(w, gamma, S, Q, count, eps, K)
    err = (wg[:, :, :K].double() - exact).abs()
    bound = 2.0 ** -11 * (1 + 2.0 ** -10) * exact.abs() + 2.0 ** -25
    print(f"[parity] fold_weights K={K}: wg worst |err| / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), f"wg: {(err > bound).sum().item()} elements beyond one fp16 rounding, worst ratio {(err / bound).max().item():.3f}"
    ref_bg, mag = R.fold_bias(w, bi, beta, wg, mean_k, K)
    berr = (bg - ref_bg).abs()
    bbound = K * 2.0 ** -24 * mag
    print(f"[parity] fold_weights K={K}: bg worst |err| / bound {(berr / bbound).max().item():.3f}")
    assert (berr <= bbound).all(), f"bg: worst |err| / (K 2^-24 sum|terms|) {(berr / bbound).max().item():.3f}"


# ---------------------------------------------------------------- 6: refusals
def test_bad_arguments():
    """every refusal of the entry points returns MOCA_E_BADARG and leaves a sentinel-filled output (and the accumulators) untouched"""
    l = L.load()
    F, HW, Cn = 4, 16, 64
    x = torch.zeros(F * HW * 512, dtype=torch.float16, device=DEV)
    y = torch.full_like(x, R.SENTINEL)
    gm = torch.ones(260, dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    cs = torch.zeros(1 << 14, dtype=torch.float32, device=DEV)
    gs = torch.full((F * 64,), 5, dtype=torch.int64, device=DEV)
    gs2 = gs.clone()
    p = L.ptr
    off4 = C.c_void_p(gm.data_ptr() + 4)                     # a float pointer that is not 16-byte aligned
    eps = C.c_float(1e-5)

    def gn(F=F, HW=HW, Cn=Cn, fps=1):
        return l.moca_groupnorm_nhwc_f16(p(x), p(y), p(gm), p(gm), F, HW, Cn, fps, eps, 1, p(ws), None)

    def gst(F=F, HW=HW, Cn=Cn, fps=1, gamma=p(gm), beta=p(gm)):
        return l.moca_groupnorm_gstat_f16(p(x), p(y), gamma, beta, p(gs), F, HW, Cn, fps, eps, 1, None)

    def col(F=F, HW=HW, Cn=Cn, fps=1, tile=16):
        return l.moca_groupnorm_colsum_f16(p(x), p(y), p(gm), p(gm), p(cs), tile, F, HW, Cn, fps, eps, 1, p(ws), None)

    def cat(F=F, HW=HW, C1=32, C2=32, fps=1, Fb=0, b=True, gamma=p(gm), beta=p(gm)):
        return l.moca_groupnorm_gstat_cat_f16(p(x), p(x), p(y), gamma, beta, p(gs), p(gs2) if b else None, Fb, F, HW, C1, C2, fps, eps, 1, None)

    def con(F=F, HW=HW, C1=32, C2=32, fps=1):
        return l.moca_concat_channels_gstat_f16(p(x), p(x), p(y), F, HW, C1, C2, fps, p(gs), None)

    def acc(F=F, HW=HW, Cn=Cn, fps=1, cpg=2, coff=0):
        return l.moca_gstat_accum_f16(p(x), F, HW, Cn, fps, cpg, coff, p(gs), None)

    bad = {
        "groupnorm F % fps": gn(fps=3), "groupnorm C % 32": gn(Cn=48), "groupnorm C % 8": gn(Cn=36), "groupnorm fps 0": gn(fps=0),
        "groupnorm C / 8 > 1024": gn(F=1, HW=1, Cn=8224),
        "gstat F % fps": gst(fps=3), "gstat C % 32": gst(Cn=48), "gstat C % 8": gst(Cn=36), "gstat gamma misaligned": gst(gamma=off4),
        "gstat beta misaligned": gst(beta=off4),
        "colsum F % fps": col(fps=3), "colsum C % 32": col(Cn=48), "colsum tile straddles": col(tile=12), "colsum tile 0": col(tile=0),
        "cat F % fps": cat(fps=3), "cat C % 32": cat(C1=32, C2=16, b=False), "cat C1 % 8": cat(C1=36, C2=28), "cat gamma misaligned": cat(gamma=off4),
        "cat beta misaligned": cat(beta=off4), "cat b's groups do not nest": cat(C1=64, C2=96), "cat b's C2 % 32": cat(C1=40, C2=24),
        "cat Fb > F": cat(Fb=8), "cat F % Fb": cat(Fb=3), "cat Fb % fps": cat(fps=2, Fb=1),
        "concat C % 32": con(C1=8, C2=8), "concat F % fps": con(fps=3), "concat C1 % 8": con(C1=36, C2=28),
        "accum last group >= 32": acc(Cn=320, cpg=10, coff=8), "accum coff < 0": acc(coff=-8), "accum cpg 0": acc(cpg=0), "accum C % 8": acc(Cn=36),
        "accum F % fps": acc(fps=3),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in bad.items() if v != -1}
    assert not wrong, f"accepted (or failed otherwise): {wrong}"
    assert (y == R.SENTINEL).all() and (gs == 5).all(), "a refused call wrote to its output"
    # the same calls without the flaw are accepted
    assert gn() == 0 and gst() == 0 and col() == 0 and cat(b=False) == 0 and cat(C1=64, C2=64, Fb=2) == 0 and con() == 0 and acc() == 0
    assert acc(Cn=320, cpg=10, coff=0) == 0
