"""GPU: every kernel of csrc/attention.hip (and the head-dim-80 kernel, which shares the transposing LDS read) computes the bits the
parent commit computed.  tests/golden/attention_parent_sha.npz holds the sha256 of the outputs of the parent commit's library on the
cases of tests/attention_edges_ref.py::PARENT_CASES -- host-generated operands, outputs pre-filled with NaN so that an unwritten row
changes the hash -- recorded by tools/record_parent_fixtures.py --attention-sha from a checkout of that commit.  The requirement is
equality, case by case; tests/test_attention_edges_gpu.py holds the same routes to a float64 reference."""
import pytest
import torch

import attention_edges_ref as R
from helpers import golden

pytestmark = pytest.mark.gpu

from moca_video_amd import ops  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    g = golden("attention_parent_sha")
    want = {str(n): str(s) for n, s in zip(g["names"], g["sha256"])}
    assert sorted(want) == sorted(c[1] for c in R.PARENT_CASES), "the fixture does not hold exactly the cases of PARENT_CASES"
    return want


@pytest.mark.parametrize("route", R.PARENT_ROUTES)
def test_outputs_keep_the_parent_commits_bits(route, recorded):
    ops.set_stream(None)
    differ = []
    for _, name, kind, p in (c for c in R.PARENT_CASES if c[0] == route):
        out = R.run_parent_case(ops, name, kind, p)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any(), f"{name}: an output row was not written"
        got = R.sha(out)
        print(f"[parent sha] {route} {name}: {'equal' if got == recorded[name] else 'DIFFERS'}")
        if got != recorded[name]:
            differ.append(name)
    assert not differ, f"{route}: outputs differ from the parent commit's on {differ}"
