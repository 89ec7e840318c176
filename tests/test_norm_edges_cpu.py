"""CPU half of the norm edge suite (tests/norm_edges_ref.py, tests/test_norm_edges_gpu.py): the queries the GPU file relies on agree with
the restated dispatch, every case of the table is on the route it names, every case tells every wrong restatement that applies to it
from the reference under the per-block metric (so no shape is too small or too symmetric), and every norm-family launch of the
fixture plans belongs to a class the GPU table runs."""
import pytest
import torch

import norm_edges_ref as R
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


def _rows_with_chunks(n, vpr):
    """row counts around n chunks of 16 bytes at vpr chunks per row"""
    return {max(r, 1) for r in ((n - 1) // vpr, n // vpr, n // vpr + 1, -(-n // vpr))}


def test_queries_equal_the_restated_dispatch(tune):
    """ops.groupnorm_route / ops.groupnorm_nchunk against route_restated / nchunk_restated over (F, HW, C, fps, knob): every channel
    width of the table, the chunk-count boundaries 255 | 256, 1024 | 1025, 2048 | 2049, 3072 | 3073, 4096 | 4097, cpg 128 | 136, the 8 MiB
    and 28 MiB size rules on either side, and every refusal"""
    seen = set()
    shapes = set()
    for C in (32, 64, 96, 128, 256, 320, 384, 640, 960, 1280, 2048, 2560, 4096, 4352, 8192):
        cpg = C // 32
        for F, fps in ((1, 1), (2, 1), (4, 2), (16, 16), (16, 1), (32, 1)):
            for HW in (1, 3, 8, 37, 160, 161, 1024, 4097):
                shapes.add((F, HW, C, fps))
            if cpg % 8 == 0:
                for n in (255, 256, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097):
                    for R_ in _rows_with_chunks(n, cpg // 8):
                        if R_ % fps == 0 or fps == 1:
                            shapes.add((F, max(R_ // fps, 1), C, fps))
            for lim in (8 << 20, 28 << 20):                       # F HW C 2 bytes on either side of the size rules
                for HW in {max(lim // (F * C * 2) + d, 1) for d in (-1, 0, 1)} | {160, 161}:
                    shapes.add((F, HW, C, fps))
    shapes |= {(0, 8, 64, 1), (4, 0, 64, 1), (4, 8, 0, 1), (4, 8, 72, 1), (4, 8, 48, 1), (4, 8, 64, 0), (4, 8, 64, 3), (1, 8, 8224, 1),
               (1, 1 << 24, 64, 1), (1, (1 << 24) - 1, 64, 1)}
    for knob in (0, 1, 2):
        tune(L.MOCA_TUNE_GN_SLAB, knob)
        for F, HW, C, fps in sorted(shapes):
            got, want = ops.groupnorm_route(F, HW, C, fps), R.route_restated(F, HW, C, fps, knob)
            assert got == want, f"route of F={F} HW={HW} C={C} fps={fps} knob={knob}: query {got}, restated {want}"
            seen.add(got)
    assert seen == set(R.ROUTE_NAME) | {0}
    for F in (0, 1, 2, 3, 4, 12, 16, 100, 2047, 2048, 2049, 5000):
        for HW in (0, 1, 7, 8, 9, 57, 100, 1360, 4097, 65535, 65536):
            assert ops.groupnorm_nchunk(F, HW) == R.nchunk_restated(F, HW), (F, HW)
    assert ops.groupnorm_route(4, 100, 4352, 1) == L.MOCA_GN_ROUTE_STREAM and ops.groupnorm_route(4, 100, 4096, 1) != L.MOCA_GN_ROUTE_STREAM


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c["entry"] == "groupnorm"])
def test_case_is_on_its_route(name, tune):
    c = R.CASES[name]
    tune(L.MOCA_TUNE_GN_SLAB, c["knob"])
    assert R.ROUTE_NAME.get(R.case_route(c)) == c["route"], name


def test_table_reaches_every_class_the_issue_names(tune):
    """routes and template arguments; slab geometry (S clamped, empty last splits, vpr 1 / 3 / 5, cpg 128); streaming chunk classes under
    knob 0: rows per thread per chunk 0, 1-3, 4, 5-7, >= 8 at ppb 1, 3, 6, 64; one chunk; short and one-row last chunk; empty chunks;
    finalize over more than 1024 partials and over a count that is no multiple of 256"""
    gn = [c for c in R.CASES.values() if c["entry"] == "groupnorm"]
    assert {c["route"] for c in gn} == set(R.ROUTE_ID)
    slabs = []
    for c in gn:
        tune(L.MOCA_TUNE_GN_SLAB, c["knob"])
        if c["route"] in ("slab2", "slab4", "slab8"):
            slabs.append((c, R.slab_geom(c["F"], c["HW"], c["C"], c["fps"], R.case_route(c))))
    assert any(s["S"] == s["R"] < 16 for _, s in slabs)                                    # S clamped to R
    assert any(len(R.split_bounds(s)) < s["S"] for _, s in slabs)                          # the last splits are empty
    assert any(s["R"] % s["S"] for _, s in slabs)
    assert {1, 3, 5} <= {s["vpr"] for _, s in slabs} and any(c["C"] == 4096 for c, _ in slabs)
    classes, ppbs, single, short_last, one_row_last, empty, partials = set(), set(), False, False, False, False, set()
    tune(L.MOCA_TUNE_GN_SLAB, 0)
    for c in gn:
        if c["knob"] != 0:
            continue
        g = R.chunk_geom(c["F"], c["HW"], c["C"])
        b = R.chunk_bounds(c["HW"], g)
        ppbs.add(g["ppb"])
        single |= g["nchunk"] == 1
        short_last |= len(b) > 1 and b[-1][1] - b[-1][0] < g["pc"]
        one_row_last |= len(b) > 1 and b[-1][1] - b[-1][0] == 1
        empty |= g["live"] < g["nchunk"]
        partials.add(c["fps"] * g["nchunk"])
        for lo, hi in b:
            for py in range(g["ppb"]):
                n = R.rows_of_thread(hi - lo, g["ppb"], py)
                classes.add("0" if n == 0 else "1-3" if n < 4 else "4" if n == 4 else "5-7" if n < 8 else ">=8")
    assert classes == {"0", "1-3", "4", "5-7", ">=8"} and ppbs == {1, 3, 6, 64}
    assert single and short_last and one_row_last and empty
    assert any(n > 1024 and n % 256 == 0 for n in partials) and any(n > 1024 and n % 256 for n in partials)
    c = R.CASES["gn_stream_k0_4x4097x32_fps1"]
    g = R.chunk_geom(4, 4097, 32)
    assert (g["nchunk"], g["pc"], g["live"]) == (512, 9, 456)
    for c in R.CASES.values():
        if c["entry"] in ("concat", "accum"):
            assert R.grid_exact(c), c["name"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_tells_every_mutation(name, tune):
    """the reference restated from sums equals the two-pass reference; each wrong restatement that applies to the case moves some
    (statistics group, channel group) block beyond TOL16 in some round.  Accumulator cases (exact grids): it changes an integer."""
    c = R.CASES[name]
    if c["entry"] == "groupnorm":
        tune(L.MOCA_TUNE_GN_SLAB, c["knob"])
    muts = R.mutations_of(c)
    assert muts and set(muts) <= set(R.MUTATIONS)
    pending = set(muts)
    for rnd in range(R.n_rounds(c)):
        inp = R.spike_input(c, rnd)
        ref = R.reference(*inp, c["fps"], silu=c["silu"])
        assert R.block_errors(R.restated(c, inp), ref, c["fps"]).max() < 1e-6, f"{name}: the sums restatement is not the reference"
        for m in sorted(pending):
            if R.block_errors(R.restated(c, inp, m), ref, c["fps"]).max() > R.TOL16:
                pending.discard(m)
    assert not pending, f"{name}: not told from the reference: {sorted(pending)}"
    if c["entry"] in ("concat", "accum"):
        Cn, cpg, coff = c.get("Cn", c["C"]), c.get("cpg", c["C"] // 32), c.get("coff", 0)
        x = R.grid_input(c["F"], c["HW"], Cn, R.seed_of(name))
        right = R.to_fixed(*R.stats_sums(x, c["fps"], cpg, coff))
        S, Q = R.stats_sums(x, c["fps"], cpg, coff)
        assert torch.equal(S * R.SUM_SCALE, torch.round(S * R.SUM_SCALE)) and torch.equal(Q * R.SQ_SCALE, torch.round(Q * R.SQ_SCALE))
        n_sg = c["F"] // c["fps"]
        for m in muts:
            if m in ("silu_dropped",):
                continue
            w = R.row_weights(c["F"], c["HW"], Cn, m) if m.startswith(("drop_", "chunk_")) else None
            cw = cpg + 1 if m == "cpg_plus_1" else cpg - 1 if m == "cpg_minus_1" else cpg
            fw = c["fps"] + 1 if m == "fps_plus_1" else c["fps"] - 1 if m == "fps_minus_1" else c["fps"]
            wrong = R.to_fixed(*R.stats_sums(x, fw, cw, 0 if m == "coff_ignored" else coff, w, n_sg))
            assert not torch.equal(wrong, right), f"{name}: the exact grid does not tell {m}"


def test_census_of_the_fixture_plans_is_inside_the_table():
    """every groupnorm / groupnorm_gstat / groupnorm_colsum / groupnorm_gstat_cat / concat_channels_gstat / gstat_accum launch of the plans
    of plan_cpu.FULL_PLANS, classified through the queries (default knobs), is of a class the GPU table runs: a plan change that moves
    a launch onto an untested route, template argument or grouping fails here"""
    from helpers import FULL
    from plan_cpu import FULL_PLANS
    from moca_video_amd import UNetModel
    from moca_video_amd.plan import _Plan
    table = R.table_classes()
    m = UNetModel(**FULL)
    dev = torch.device("cpu")
    m._pack(dev)
    seen, missing = {}, {}
    for tag, args, kw in FULL_PLANS:
        for s in _Plan(m, *args, torch.float32, dev, **kw).steps:
            cls = R.launch_class(s.func.__name__, s.args, s.keywords)
            if cls is None:
                continue
            seen[cls] = seen.get(cls, 0) + 1
            if cls not in table:
                missing.setdefault(cls, []).append(tag)
    for cls, n in sorted(seen.items(), key=str):
        print(f"[census] {n:4d} x {cls}")
    assert not missing, f"norm-family launches of the plans outside the GPU table: { {k: sorted(set(v)) for k, v in missing.items()} }"
    routes = {cls[1] for cls in seen if cls[0] == "groupnorm"}
    assert {"slab4", "slabreg2"} <= routes                    # routes the plans launch that only this suite runs per kernel
