"""CPU: temporal attention over 17 .. 32 frames -- the refusals of the C-ABI entry moca_temporal_attention_long_f16 (nothing is
launched), the ISA of its two instantiations, what a plan RECORDS for T > 16 (plans built on the host: the launch list is read, nothing
runs), and the FIFO entry points' refusal of windows longer than 16 frames."""
import ctypes as C
import os
import shutil
import sys
import types

import pytest

from helpers import REDUCED
from plan_cpu import cpu_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- C-ABI
def test_abi_entry_refusals():
    """every refusal differs from the acceptable call in ONE argument and returns MOCA_E_BADARG (-1) before any launch.  (The
    acceptable call itself is not made here: it would launch.)"""
    from moca_video_amd import lib
    f = lib.load().moca_temporal_attention_long_f16
    ok = dict(q=0x10000, k=0x20000, v=0x30000, out=0x40000, B=1, T=24, HW=4, heads=2, ld_qkv=384, ldo=128, scale=0.125, causal=0)

    def call(**kw):
        a = dict(ok, **kw)
        ptr = lambda x: None if x is None else C.c_void_p(x)
        return f(ptr(a["q"]), ptr(a["k"]), ptr(a["v"]), ptr(a["out"]), a["B"], a["T"], a["HW"], a["heads"], a["ld_qkv"], a["ldo"],
                 a["scale"], a["causal"], None)
    for bad in (dict(T=16), dict(T=33), dict(T=0), dict(q=None), dict(k=None), dict(v=None), dict(out=None),
                dict(q=0x10008), dict(k=0x20008), dict(v=0x30008), dict(out=0x40004), dict(ld_qkv=388), dict(ldo=130),
                dict(ld_qkv=120), dict(ldo=124), dict(causal=2), dict(causal=-1), dict(causal=1, scale=0.0), dict(causal=1, scale=-0.125),
                dict(B=0), dict(HW=0), dict(heads=0)):
        assert call(**bad) == -1, bad
    assert lib.SIGNATURES["moca_temporal_attention_long_f16"][1][-2:] == [C.c_int32, C.c_void_p]


# ---------------------------------------------------------------- ISA
def test_isa_of_the_long_kernels():
    """both instantiations exist, spill nothing and use no scratch; the mask is one comparison per score register in both, so the
    causal one has the MFMAs and no more VGPRs than the plain one"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from moca_video_amd import lib
    if not os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")) or shutil.which("c++filt") is None:
        pytest.skip("llvm-objdump / c++filt not available")
    r = isa_report.analyse(lib.LIB_PATH)
    tl = {k: v for k, v in r.items() if "tattn_long_kernel" in k}
    assert len(tl) == 2, sorted(tl)
    plain = next(v for k, v in tl.items() if "<false>" in k or "ILb0E" in k)
    caus = next(v for k, v in tl.items() if "<true>" in k or "ILb1E" in k)
    for v in (plain, caus):
        assert v["scratch"] == 0 and v["vgpr_spill_count"] == 0
    assert caus["mfma_total"] == plain["mfma_total"] > 0
    assert caus["vgpr_count"] <= plain["vgpr_count"]


# ---------------------------------------------------------------- what a plan records
def _names(plan):
    out = []
    for s in plan.steps:
        n = s.func.__name__
        if n == "gemm" and s.keywords.get("tattn") is not None:
            n = "gemm:tattn"
        out.append(n)
    return out


def test_plan_records_the_long_kernel_past_16_frames():
    _, pl = cpu_plan(REDUCED, 1, 24, 16, 16, 77)
    n = _names(pl)
    assert n.count("temporal_attention_long") == 2 * 17                     # attn1 and attn2 of 17 temporal blocks
    assert not {"temporal_attention", "temporal_attention_causal", "gemm:tattn"} & set(n)
    long_steps = [s for s in pl.steps if s.func.__name__ == "temporal_attention_long"]
    assert all(s.keywords["T"] == 24 and s.keywords["causal"] is False and s.keywords["B"] == 1 for s in long_steps)
    assert sorted({s.keywords["HW"] for s in long_steps}) == [4, 16, 64, 256]


def test_causal_plan_records_the_mask():
    _, pl = cpu_plan(dict(REDUCED, use_causal_attention=True, temporal_length=24), 1, 24, 16, 16, 77)
    long_steps = [s for s in pl.steps if s.func.__name__ == "temporal_attention_long"]
    assert len(long_steps) == 2 * 17 and all(s.keywords["causal"] is True for s in long_steps)
    assert not {"temporal_attention", "temporal_attention_causal", "gemm:tattn"} & set(_names(pl))


@pytest.mark.parametrize("T", [16, 8])
def test_up_to_16_frames_nothing_changes(T):
    _, pl = cpu_plan(REDUCED, 1, T, 16, 16, 77)
    n = _names(pl)
    assert "temporal_attention_long" not in n
    assert n.count("temporal_attention") + n.count("gemm:tattn") == 2 * 17


def test_refusals_of_the_plan():
    with pytest.raises(ValueError, match=r"T = 33"):
        cpu_plan(REDUCED, 1, 33, 16, 16, 77)
    with pytest.raises(ValueError, match=r"T = 24 .*temporal_length = 16"):
        cpu_plan(dict(REDUCED, use_causal_attention=True), 1, 24, 16, 16, 77)
    with pytest.raises(ValueError, match=r"hw = 256 .*T = 24"):       # 16 x 16 latents: already the first level is no multiple of 24
        cpu_plan(dict(REDUCED, temporal_selfatt_only=False), 1, 24, 16, 16, 77)


def test_statistics_range_check_of_the_plan():
    """a (statistics group, channel group) accumulator takes fewer than 2^11 partials (csrc/common.h): 32 frames of 64 x 64 latents
    are inside (1640 partials by the plan's bound, 2 x ceil(rows / 160): it counts 160-row tiles whatever the route; the launch itself
    takes 256-row tiles there, 1024 partials, the figure of common.h), the first row count past 1023 tiles of 160 rows is refused --
    by the function.  The plan asks it for groups of more than 16 frames only: every plan of up to 16 frames is built as before"""
    from moca_video_amd import plan
    plan._check_gstat_range(32 * 2560)
    plan._check_gstat_range(32 * 4096)
    plan._check_gstat_range(1023 * 160)
    with pytest.raises(ValueError, match="statistics"):
        plan._check_gstat_range(1023 * 160 + 1)
    with pytest.raises(ValueError, match="statistics"):
        plan._check_gstat_range(32 * 72 * 72)
    # in a plan: 144 x 144 latents, whose second level (72 x 72 pixels, 128 channels) takes the fixed-point statistics
    with pytest.raises(ValueError, match="statistics over 165888 rows"):
        cpu_plan(REDUCED, 1, 32, 144, 144, 77)
    _, pl = cpu_plan(REDUCED, 1, 16, 208, 208, 77)                 # 16 x 10 816 = 173 056 rows at that level: recorded as before
    assert any(s.func.__name__ == "groupnorm_gstat" and s.keywords["frames_per_stat"] == 16 and s.keywords["HW"] == 10816 for s in pl.steps)


# ---------------------------------------------------------------- FIFO stays at 16 frames
def test_fifo_entry_points_refuse_longer_windows_up_front():
    """before the model, the conditioning or the GPU are touched (they are None here)"""
    from moca_video_amd.fifo import fifo_ddim_sampling, fifo_ddim_sampling_multiprompts
    from moca_video_amd.fifo_graph import FifoEngine
    args = types.SimpleNamespace(num_inference_steps=48, video_length=24, lookahead_denoising=True, num_partitions=2, new_video_length=10)
    with pytest.raises(ValueError, match="video_length"):
        fifo_ddim_sampling(args, None, None, (1, 4, 24, 8, 8), None)
    with pytest.raises(ValueError, match="video_length"):
        fifo_ddim_sampling_multiprompts(args, None, None, (1, 4, 24, 8, 8), None, ["a", "b", "5,5"])
    with pytest.raises(ValueError, match="video_length"):
        FifoEngine(args, None, None, None, None, 1.0, None)
