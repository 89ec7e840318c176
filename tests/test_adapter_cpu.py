"""CPU: the adapter-guided forward (`features_adapter`, openaimodel3d.py:555-567) as far as it can be checked without a GPU -- the C-ABI
entry moca_nchw_add_rows_f16 and its argument validation, what a plan RECORDS with and without the maps (plans built on the host: the
launch list is read, nothing runs), the reference's failure modes for a wrong list, the refusals, and the sensitivity of the goldens
(tools/make_golden_adapter.py)."""
import ctypes as C
import difflib
import inspect
import os
import re
import types

import pytest
import torch

from helpers import FULL, REDUCED, golden, relerr
from plan_cpu import cpu_plan, signature
from test_unet_gpu import TOL_UNET
import adapter_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADD = "nchw_add_rows"


# ---------------------------------------------------------------- C ABI
def test_add_rows_symbol_and_argument_validation():
    """moca_nchw_add_rows_f16 is declared (citing the reference lines), exported, mirrored in ctypes and wrapped, and every bad argument
    returns MOCA_E_BADARG before a launch (no GPU here: a launch would fail differently)"""
    from moca_video_amd import lib, ops
    l = lib.load()
    hdr = open(os.path.join(ROOT, "include", "moca_hip.h")).read()
    assert re.search(r"openaimodel3d\.py:562-564[^/]*\*/\s*int\s+moca_nchw_add_rows_f16\s*\(", hdr, re.S)
    assert hasattr(l, "moca_nchw_add_rows_f16") and "moca_nchw_add_rows_f16" in lib.SIGNATURES and callable(ops.nchw_add_rows)
    f = l.moca_nchw_add_rows_f16
    p = lambda v=64: C.c_void_p(v)
    good = dict(rows=p(), src=p(), f32=1, F=4, Fsrc=2, C=64, HW=35, ld=192)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["rows"], a["src"], a["f32"], a["F"], a["Fsrc"], a["C"], a["HW"], a["ld"], None)
    cases = [dict(rows=None), dict(src=None), dict(F=0), dict(F=-2), dict(C=0), dict(C=-64), dict(HW=0), dict(HW=-1), dict(Fsrc=0),
             dict(Fsrc=-1), dict(Fsrc=3), dict(F=3, Fsrc=2), dict(ld=63), dict(ld=0), dict(C=256),
             dict(rows=p(72)),                                 # the rows are accessed 16 bytes at a time
             dict(C=60, ld=60), dict(ld=68)]                   # ... so 8 channels per access and row starts that stay aligned
    for kw in cases:
        assert call(**kw) == -1, kw
        assert call(f32=0, **kw) == -1, kw
    assert call(src=p(66)) == -1 and call(src=p(65), f32=0) == -1         # the source is read by elements: aligned to its type


# ---------------------------------------------------------------- recorded plans
def _ends_of_input_blocks(build):
    """build() a plan while recording len(plan.steps) behind every `run_seq`: call k (k >= 1) is input block k"""
    from moca_video_amd.plan import _Plan
    ends, orig = [None], _Plan.run_seq

    def run_seq(self, seq, h):
        out = orig(self, seq, h)
        ends.append(len(self.steps))
        return out
    _Plan.run_seq = run_seq
    try:
        plan = build()
    finally:
        _Plan.run_seq = orig
    return plan, ends


def _norm(line):
    """a launch without the statistics its producer was asked to leave behind"""
    return re.sub(r"(gstat=\([^)]*\),|slabs=True,|colsum=t[0-9x]+,)", "", line)


def test_full_plans_with_and_without_the_maps():
    """FULL at the headline shape, the plain B = 1 forward and the shared-prefix guidance pair (one packing of the full-width tree
    serves the four plans, ~20 s).
    Without `adapter`: launch for launch the parent commit's list (tests/golden/plan_full_launches.npz).
    With it: that list plus exactly four nchw_add_rows, each directly behind the last launch of input blocks 2 / 5 / 8 / 11, on maps of
    320 / 640 / 1280 / 1280 channels at H x W .. H/8 x W/8 read through Fsrc = Bx * T frames.  The statistics of the pre-add tensor are
    DROPPED: the launch in front of an add carries no colsum / gstat / deferred split-K reduce, and the only other
    differences are the consumers' own statistics passes, named here: `gstat_accum` where an output block reads a site's map as the
    skip half of a virtual concat, and `groupnorm` (own reduce + plain GroupNorm) in place of `gemm_splitk_groupnorm` behind block 11."""
    from moca_video_amd import UNetModel
    from moca_video_amd.plan import _Plan
    g = golden("plan_full_launches")
    m = UNetModel(**FULL)
    dev = torch.device("cpu")
    m._pack(dev)
    assert m.adapter_sites == 4
    for tag, args, kw in (("b1_77", (1, 16, 40, 64, 77), {}), ("cfg_shared", (2, 16, 40, 64, ((1, 77), (1, 77))), dict(shared_x=True))):
        base = signature(_Plan(m, *args, torch.float32, dev, **kw))
        assert base == [str(s) for s in g[tag]], f"{tag}: a plan without adapter must record the parent commit's launches"
        plan, ends = _ends_of_input_blocks(lambda: _Plan(m, *args, torch.float32, dev, adapter=4, **kw))
        sig = signature(plan)
        at = [i for i, s in enumerate(plan.steps) if s.func.__name__ == ADD]
        assert at == [ends[k] for k in (2, 5, 8, 11)], (tag, at, ends)
        F = args[0] * 16
        want = [(320, 40, 64), (640, 20, 32), (1280, 10, 16), (1280, 5, 8)]
        assert [tuple(t.shape) for t in plan.adapter_in] == [(16,) + w for w in want]
        assert all(t.dtype == torch.float32 for t in plan.adapter_in)
        for i, (Cn, H, W), src in zip(at, want, plan.adapter_in):
            s, prod = plan.steps[i], plan.steps[i - 1]
            assert s.args[1] is src and s.keywords == dict(F=F, Fsrc=16, Cn=Cn, HW=H * W), (tag, s.keywords)
            assert tuple(s.args[0].shape) == (F * H * W, Cn)
            # the producer of h: the GEMM that wrote the rows the add updates, back on its plain store loop and its own reduce
            assert prod.func.__name__ == "gemm" and prod.args[2].data_ptr() == s.args[0].data_ptr()
            assert all(prod.keywords.get(k) is None for k in ("colsum", "gstat", "rowsum")) and not prod.keywords.get("slabs")
        extra = []
        sm = difflib.SequenceMatcher(a=[_norm(s) for s in base], b=[_norm(s) for s in sig], autojunk=False)
        for op, i1, i2, j1, j2 in sm.get_opcodes():
            if op == "equal":
                continue
            gone, new = [s.split("(")[0] for s in base[i1:i2]], [s.split("(")[0] for s in sig[j1:j2]]
            assert gone in ([], ["gemm_splitk_groupnorm"]), (tag, base[i1:i2], sig[j1:j2])
            extra += [n for n in new if n != ADD]
            if gone:
                assert new == [ADD, "groupnorm"], (tag, new)
        assert sorted(set(extra)) == ["groupnorm", "gstat_accum"] and extra.count("groupnorm") == 1 and 1 <= extra.count("gstat_accum") <= 4, extra
        assert len(sig) == len(base) + 4 + len(extra) - 1


def test_reduced_plan_sites_and_set_adapter_shapes():
    """the site list comes from the module list (the REDUCED model: 64 / 128 / 256 / 256 channels); set_adapter copies exact shapes in
    fp32 or fp16 and refuses everything else with ValueError -- the reference's `h + feat` would broadcast a [1, C, 1, 1] entry"""
    m, plan = cpu_plan(REDUCED, 2, 4, 16, 16, ((1, 77), (1, 77)), shared_x=True, adapter=4)
    shapes = [(4,) + s for s in AR.sites(64, [1, 2, 4, 4], 16, 16)]
    assert [tuple(t.shape) for t in plan.adapter_in] == shapes and plan.adapter_sites == [2, 5, 8, 11]
    adds = [s for s in plan.steps if s.func.__name__ == ADD]
    # (the shared prefix ends at the first cross-attention, in input block 1: both branches exist at every site and read the same 4 frames)
    assert [s.keywords["F"] for s in adds] == [8, 8, 8, 8] and all(s.keywords["Fsrc"] == 4 for s in adds)
    good = [torch.randn(s) for s in shapes]
    plan.set_adapter(good)
    assert all(torch.equal(a, b) for a, b in zip(plan.adapter_in, good))
    plan.set_adapter([t.half() for t in good])
    assert all(torch.equal(a, b.half().float()) for a, b in zip(plan.adapter_in, good))
    for k, bad in ((0, torch.zeros(1, 64, 1, 1)), (1, torch.zeros(4, 128, 8, 9)), (2, torch.zeros(8, 256, 4, 4)), (3, torch.zeros(4, 256, 2)),
                   (0, torch.zeros(shapes[0], dtype=torch.float64)), (1, torch.zeros(shapes[1], dtype=torch.bfloat16))):
        with pytest.raises(ValueError, match=rf"features_adapter\[{k}\]"):
            plan.set_adapter(good[:k] + [bad] + good[k + 1:])
    with pytest.raises(ValueError):
        plan.set_adapter(good[:3])
    from moca_video_amd.plan import _Plan
    with pytest.raises(ValueError, match="adapter sites"):
        _Plan(m, 1, 4, 16, 16, 77, torch.float32, torch.device("cpu"), adapter=3)
    _, plain = cpu_plan(REDUCED, 1, 4, 16, 16, 77)
    assert plain.adapter_in is None and not any(s.func.__name__ == ADD for s in plain.steps)
    with pytest.raises(ValueError):
        plain.set_adapter(good)


# ---------------------------------------------------------------- public surface
def test_wrong_list_length_keeps_the_references_errors_and_the_refusals():
    """openaimodel3d.py:563,566-567: too few maps fail at `features_adapter[adapter_idx]` (IndexError), too many at the assert behind
    the loop; forward_concat / forward_concurrent and the hybrid keys refuse the argument (all before anything touches a device)"""
    from moca_video_amd import DenoiseModel, UNetModel
    m = UNetModel(**REDUCED)
    x, ctx, t = torch.zeros(1, 4, 4, 16, 16), torch.zeros(1, 77, 128), torch.tensor([1])
    maps = [torch.zeros((4,) + s) for s in AR.sites(64, [1, 2, 4, 4], 16, 16)]
    for call in (lambda fa: m(x, t, context=ctx, features_adapter=fa),
                 lambda fa: m.forward_segments(x, t, [ctx, ctx], shared_x=True, features_adapter=fa),
                 lambda fa: m.forward_segments(x, t, [ctx], features_adapter=fa)):
        with pytest.raises(IndexError):
            call(maps[:3])
        with pytest.raises(IndexError):
            call([])
        with pytest.raises(AssertionError, match="Wrong features_adapter"):
            call(maps + maps[:1])
        with pytest.raises(ValueError, match="CUDA"):                # (the right count: refused for the device, like every forward)
            call(maps)
    with pytest.raises(NotImplementedError, match="features_adapter"):
        m.forward_concat(x, [torch.zeros(1, 4, 4, 16, 16)], t, context=ctx, features_adapter=maps)
    with pytest.raises(NotImplementedError, match="features_adapter"):
        m.forward_concurrent([dict(x=x, timesteps=t, context=ctx), dict(x=x, timesteps=t, context=ctx, features_adapter=maps)])
    cfg = {"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, in_channels=8)}
    for key in ("hybrid", "hybrid-adm", "hybrid-time", "hybrid-adm-mask", "hybrid-time-adm"):
        dm = DenoiseModel(cfg, conditioning_key=key)
        with pytest.raises(NotImplementedError, match="features_adapter"):
            dm.apply_model(x, t, {"c_concat": [x], "c_crossattn": [ctx]}, features_adapter=maps)


def test_sampler_and_engine_surface():
    """DDIMSampler.sample / BaseEngine take the maps; the one-graph engine stays available for a crossattn model with them and is not
    offered for a hybrid one; FIFO sampling has no such argument (out of scope)"""
    from moca_video_amd import DenoiseModel
    from moca_video_amd.fifo import fifo_ddim_sampling
    from moca_video_amd.fifo_graph import BaseEngine, FifoEngine
    from moca_video_amd.sampler import DDIMSampler
    assert "features_adapter" in inspect.signature(DDIMSampler.sample).parameters
    assert "features_adapter" in inspect.signature(BaseEngine.__init__).parameters
    assert "features_adapter" in inspect.signature(BaseEngine.reset).parameters
    assert "features_adapter" not in inspect.signature(fifo_ddim_sampling).parameters
    assert "features_adapter" not in inspect.signature(FifoEngine.__init__).parameters
    cfg = lambda c: {"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": dict(REDUCED, in_channels=c)}
    x = types.SimpleNamespace(is_cuda=True, shape=(1, 4, 8, 16, 16))
    ctx, z = torch.zeros(1, 77, 128), torch.zeros(1, 4, 8, 16, 16)
    cond = {"c_crossattn": [ctx], "fps": torch.tensor([10])}
    uc = dict(cond, c_crossattn=[ctx + 1])
    maps = [torch.zeros(8, 64, 16, 16)] * 4
    plain = DenoiseModel(cfg(4))
    assert BaseEngine.supported(plain, x, cond, uc, 12.0) and BaseEngine.supported(plain, x, cond, uc, 12.0, features_adapter=maps)
    hyb = DenoiseModel(cfg(8), conditioning_key="hybrid")
    hc, hu = dict(cond, c_concat=[z]), dict(uc, c_concat=[z])
    assert BaseEngine.supported(hyb, x, hc, hu, 12.0) and not BaseEngine.supported(hyb, x, hc, hu, 12.0, features_adapter=maps)


# ---------------------------------------------------------------- goldens
def test_goldens_hold_what_the_gpu_tests_need():
    """unet_reduced_adapter.npz / unet_full_adapter.npz: outputs and call metadata only; the maps are regenerated by name
    (tests/adapter_ref.py) at the per-site scales the fixture records -- the size of the reference's h there, so growing over the
    sites -- and the two outputs of the guidance pair differ by far more than the tolerance they are compared under.  (That dropping
    the maps moves the reference's output by > 20 x TOL_UNET and that the GroupNorm statistics move by >= 25 % at every site is
    asserted on the reference by tools/make_golden_adapter.py, which cannot run here.)"""
    g = golden("unet_reduced_adapter")
    for name, shape in (("two", (2, 4, 4, 16, 16)), ("fifo", (1, 4, 16, 8, 40)), ("cfg", (1, 4, 16, 8, 40)), ("cfg_uc", (1, 4, 16, 8, 40))):
        assert g[name].shape == shape
    assert len(g["fifo__t"]) == 16 and int(g["fifo__L"]) == 154 and int(g["two__L"]) == 77 == int(g["cfg__L"])
    for name in ("two", "fifo", "cfg"):
        sc = g[name + "__scale"]
        assert sc.shape == (4,) and (sc > 1.0).all() and (sc[1:] > sc[:-1]).all()
    assert relerr(g["cfg_uc"], g["cfg"]) > 20 * TOL_UNET
    f = AR.features("ad", "two", 8, AR.sites(64, [1, 2, 4, 4], 16, 16), g["two__scale"])
    assert [tuple(t.shape) for t in f] == [(8, 64, 16, 16), (8, 128, 8, 8), (8, 256, 4, 4), (8, 256, 2, 2)]
    assert all(t.mean(dim=(0, 2, 3)).abs().min() > 0 for t in f) and not torch.equal(f[0][:4], f[0][4:])
    gf = golden("unet_full_adapter")
    assert gf["fifo16"].shape == (1, 4, 16, 40, 64) and gf["fifo16__scale"].shape == (4,) and int(gf["fifo16__L"]) == 77
