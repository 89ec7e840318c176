"""GPU: every kernel of the GroupNorm family of csrc/norm.hip computes the bits the parent commit computed.
tests/golden/norm_parent_sha.npz holds the sha256 of what the parent commit's library left on the cases of
tests/norm_edges_ref.py::parent_names -- every case of CASES on its plain and on its first spike input with the case's
MOCA_TUNE_GN_SLAB knob, the three fold-weights cases, and the 128 MiB shape that reaches the non-temporal-store instantiations; host-generated
operands, outputs pre-filled with the sentinel, the accumulators of the concat / accum launches non-zero before the launch and hashed
too -- recorded by tools/record_parent_fixtures.py --norm-sha from a checkout of that commit.  The kernels are deterministic (partials
combined in a fixed order, integer accumulators), so the requirement is equality, case by case; tests/test_norm_edges_gpu.py holds the
same launches to a float64 reference."""
import pytest
import torch

import norm_edges_ref as R
from helpers import golden

pytestmark = pytest.mark.gpu

from moca_video_amd import ops  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    g = golden("norm_parent_sha")
    want = {str(n): str(s) for n, s in zip(g["names"], g["sha256"])}
    assert sorted(want) == sorted(n for grp in R.PARENT_GROUPS for n in R.parent_names(grp)), "the fixture does not hold exactly the cases of parent_names"
    return want


@pytest.mark.parametrize("group", R.PARENT_GROUPS)
def test_outputs_keep_the_parent_commits_bits(group, recorded):
    ops.set_stream(None)
    got = R.parent_hashes(group)
    torch.cuda.synchronize()
    assert list(got) == R.parent_names(group)
    differ = [n for n in got if got[n] != recorded[n]]
    print(f"[parent sha] {group}: {len(got) - len(differ)} of {len(got)} equal" + (f", DIFFER: {differ}" if differ else ""))
    assert not differ, f"{group}: what the launches leave differs from the parent commit's on {differ}"
