"""Static check of the halo-tile conv kernel (csrc/gemm_halo.hip) on the cross-compiled library, as tests/test_isa_cpu.py does for the
other GEMM families: the main loop is the designed one and the anti-hoisting of the halo pieces' scalar bookkeeping still holds.

One loop body = one slice pair = 9 tap iterations of two k-tiles: 9 x 50 MFMAs, 9 x 20 fragment reads, 9 x 4 barriers.  LDS-DMA: a wave
EXECUTES 4 per iteration (36 per body); the body HOLDS 45, because the third instruction of an iteration is a W piece in waves with
wave % 4 < 2 and a halo piece in the others, and both arms of that wave-uniform branch are in the code.  No `s_waitcnt vmcnt(0)`, no LDS
write, no register-staged load in the loop; no VGPR spill, no scratch frame (what hoisting the bookkeeping out of the loop produced),
two waves per SIMD."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("gemm_w80h_kernel<64>", "gemm_w80h_kernel<32>")


@pytest.fixture(scope="module")
def isa():
    import isa_report
    from moca_video_amd import lib
    if not os.path.exists(os.path.join(isa_report.LLVM, "llvm-objdump")) or shutil.which("c++filt") is None:
        pytest.skip("llvm-objdump / c++filt not available")
    return isa_report.analyse(lib.LIB_PATH)


@pytest.mark.parametrize("name", KERNELS)
def test_halo_main_loop_is_the_designed_one(isa, name):
    assert name in isa, f"{name} is not in the library"
    d, lp = isa[name], isa[name]["loop"]
    assert lp is not None, f"{name}: no MFMA loop found"
    got = (lp["mfma"], lp["lds_dma"], lp["ds_read"], lp["barrier"])
    assert got == (450, 45, 180, 36), f"{name}: main loop (MFMA, LDS-DMA, ds_read, barriers) = {got}"
    assert lp["vmcnt0"] == 0, f"{name}: {lp['vmcnt0']} `s_waitcnt vmcnt(0)` in the main loop"
    assert lp["ds_write"] == 0 and lp["global_load"] == 0 and lp["scratch"] == 0, f"{name}: {lp}"
    assert d.get("vgpr_spill_count", 0) == 0 and d.get("private_segment_fixed_size", 0) == 0 and d["scratch"] == 0, f"{name}: spills / scratch"
    assert d["vgpr_count"] + d.get("agpr_count", 0) <= 256 and d.get("agpr_count", 0) == 0, f"{name}: registers"
