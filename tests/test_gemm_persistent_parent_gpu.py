"""GPU: the persistent GEMM kernels of csrc/gemm_persistent.hip (g4p, g4q, sqp) compute the bits the parent commit computed.
tests/golden/gemm_persistent_parent_sha.npz holds the sha256 of what the parent commit's library left on
tests/gemm_edges_ref.py::PERSISTENT_PARENT_CASES -- per route: bias x row add (rowadd_div 7 and M) x residual, `out` aliasing the
residual and GEGLU at K = 64 / 128 / 320 (one, two and five k-tile pairs) on the smallest tile count the routes take with an 8-row M tail;
the LayerNorm fold with 1, 2, 3 and 10 row partials, plain and GEGLU; a launch with prefetch blocks; sqp's contiguous walk and its 2-D
XCD partition; an output of exactly 128 MiB (the streaming stores) -- host-generated operands, the output inside a NaN-filled
allocation, recorded by tools/record_parent_fixtures.py --persistent-sha from a checkout of that commit.  The kernels have no atomics
and a fixed accumulation order (tests/test_gemm_fused_gpu.py::test_gemm_sqp_lnfold_repeatable relies on it), so the requirement is
equality, case by case; tests/test_gemm_edges_gpu.py and tests/test_gemm_fused_gpu.py hold the same launches to a float64 reference."""
import pytest
import torch

import gemm_edges_ref as R
from helpers import golden

pytestmark = pytest.mark.gpu

from moca_video_amd import ops  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    g = golden("gemm_persistent_parent_sha")
    want = {str(n): str(s) for n, s in zip(g["names"], g["sha256"])}
    assert sorted(want) == sorted(n for _, n, _ in R.PERSISTENT_PARENT_CASES), "the fixture does not hold exactly the names of PERSISTENT_PARENT_CASES"
    return want


@pytest.mark.parametrize("route", R.PARENT_ROUTES)
def test_outputs_keep_the_parent_commits_bits(route, recorded):
    ops.set_stream(None)
    got = R.persistent_parent_hashes(route)          # (asserts per case that every row was written and the canary rows are intact)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert list(got) == [n for r, n, _ in R.PERSISTENT_PARENT_CASES if r == route]
    differ = [n for n in got if got[n] != recorded[n]]
    print(f"[parent sha] {route}: {len(got) - len(differ)} of {len(got)} equal" + (f", DIFFER: {differ}" if differ else ""))
    assert not differ, f"{route}: the outputs differ from the parent commit's on {differ}"
