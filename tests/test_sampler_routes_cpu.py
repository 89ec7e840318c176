"""The sampling layer's routes against the parent commit's (tests/golden/sampler_routes.npz, recorded by
tools/record_parent_fixtures.py --samplers): which UNet entry point every guidance case reaches through `_cfg_eps`, `unet_windows` and
`_ddpm_step` and with which operands, every launch of the host-issued `sample` / `decode` loops with its coefficients, `ddim_step`,
the two queue-noising calls, two iterations of the host-driven FIFO loop, the three `supported()` predicates, the coefficient
tables, and the three trajectory engines of fifo_graph.py on a plan that holds buffers only: every launch around the forward with its
position, what each reset leaves in the state block, the plan's inputs and the tables, every refusal with its message, and which
sampler calls reuse the cached engine.  A line that differs is a behaviour change."""
import os

import numpy as np
import pytest

import sampler_routes_cpu as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_routes.npz")


@pytest.fixture(scope="module")
def now():
    return R.record()


@pytest.fixture(scope="module")
def parent():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def test_every_recorded_trace_is_still_produced(now, parent):
    assert sorted(now) == sorted(parent)
    assert len([k for k in parent if k.startswith("guidance.")]) >= 60
    assert len([k for k in parent if k.startswith("engine.")]) == 5 + 3 + 5


@pytest.mark.parametrize("group", ["guidance.cfg_eps", "guidance.windows", "guidance.ddpm", "supported", "loop", "ddim_step", "queue", "fifo", "engine.base",
                                   "engine.invert", "engine.ddpm", "engine_errors", "cache"])
def test_traces_equal_the_parents(now, parent, group):
    keys = [k for k in sorted(parent) if k.startswith(group)]
    assert keys
    for k in keys:
        assert list(now[k]) == list(parent[k]), f"{k}:\n" + "\n".join(
            f"  parent {a}\n  now    {b}" for a, b in zip(parent[k], now[k]) if a != b) + f"\n  ({len(parent[k])} lines before, {len(now[k])} now)"


def test_coefficient_tables_equal_the_parents_bit_for_bit(now, parent):
    keys = [k for k in sorted(parent) if k.startswith(("step_tables", "base_engine"))]
    assert len(keys) == 2 * (2 * 3 + 2)
    for k in keys:
        assert now[k].dtype == parent[k].dtype and now[k].shape == parent[k].shape and now[k].tobytes() == parent[k].tobytes(), k


def test_base_engine_and_step_tables_share_their_first_five_columns(now):
    for eta in ("0", "1"):
        assert now[f"base_engine.eta{eta}.rowsNone.coef"][:, :5].tobytes() == now[f"step_tables.eta{eta}.quirk1.coef"][:, :5].tobytes()
