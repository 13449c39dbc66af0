"""CPU: the table-gradient scatter's plans (tile geometry, queue capacities, workspace layout) as the workspace queries
report them, against recorded values (tests/golden/scatter_plans.json, written by tests/golden/make_scatter_plans.py).
The queries are host arithmetic and launch nothing."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scatter_plans.json")

with open(FIXTURE) as _f:
    CASES = json.load(_f)


def test_fixture_covers_the_benchmark_and_the_edges():
    shapes = {(c["num_levels"], c["log2_table_size"], c["M"]) for c in CASES}
    for grid in ((16, 19), (5, 17)):
        for M in (1048576, 393216, 196608):
            assert grid + (M,) in shapes
    assert any(c["M"] == 1 for c in CASES) and any(c["M"] % 1024 not in (0, 1) for c in CASES)
    assert any(c["log2_table_size"] < 8 and c["words"] > 0 for c in CASES)  # tile clamped to the table
    assert any(c["words"] == 0 and c["M"] > 0 for c in CASES) and any(c["producer"] == 0 and c["words"] > 0 for c in CASES)
    assert sum(c["producer"] > 0 for c in CASES) >= 5


@pytest.mark.parametrize("case", CASES, ids=[f"{i}_L{c['num_levels']}_T{c['log2_table_size']}_M{c['M']}" for i, c in enumerate(CASES)])
def test_workspace_queries_return_the_recorded_plans(case):
    from nerfstudio_amd import _native as N

    lib = N.load()
    g = N.make_grid(case["num_levels"], case["log2_table_size"], case["scalings"])
    M = case["M"]
    assert int(lib.nsamd_hashgrid_encode_bwd_workspace(g, M, 0)) == case["words"]
    assert int(lib.nsamd_hashgrid_encode_bwd_workspace(g, M, 1)) == case["words_set"]
    assert int(lib.nsamd_hashgrid_encode_bwd_workspace_state(g, M)) == case["state"]
    state = C.c_int64(-1)
    assert int(lib.nsamd_field_mlp_bwd_scatter_workspace(g, M, C.byref(state))) == case["producer"]
    assert int(state.value) == case["producer_state"]
