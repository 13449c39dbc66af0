"""CPU: the status code of entry-point calls that the argument checks answer before any HIP runtime call, against the table
recorded from the commit before the checks moved into csrc/launch.h (tests/golden/launch_checks.json, written by
tests/golden/make_launch_checks.py, which also builds the calls). Which code an input gets, and which check wins when two
fail, did not change with the move. No case reaches a launch: every recorded status is OK, INVALID_ARG or UNSUPPORTED."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

with open(os.path.join(GOLDEN, "launch_checks.json")) as _f:
    CASES = json.load(_f)

_spec = importlib.util.spec_from_file_location("make_launch_checks", os.path.join(GOLDEN, "make_launch_checks.py"))
make = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make)

ENTRY_POINTS = (
    "nsamd_hashgrid_encode_fwd", "nsamd_hashgrid_encode_bwd", "nsamd_hashgrid_encode_bwd_set", "nsamd_hashgrid_encode_bwd_gated",
    "nsamd_hashgrid_encode_bwd_rays", "nsamd_field_normals", "nsamd_density_field_fwd", "nsamd_field_mlp_bwd_scatter_phase",
    "nsamd_field_mlp_fwd", "nsamd_field_mlp_bwd", "nsamd_field_ray_terms")


def _rows(entry):
    return [c for c in CASES if c["entry"] == entry]


def test_table_is_the_generators_and_none_of_it_reaches_the_runtime():
    assert [(c["entry"], c["what"], c["set"]) for c in CASES] == [
        (entry, what, overrides) for entry, cases in make.CASES.items() for what, overrides in cases]
    assert {c["status"] for c in CASES} == {make.OK, make.INVALID, make.UNSUPPORTED}


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_table_covers_the_checks_of_every_entry_point(entry):
    rows = _rows(entry)
    sets = [c["set"] for c in rows]
    m = "num_rays" if entry == "nsamd_field_ray_terms" else "M"
    # (nsamd_hashgrid_encode_bwd_set zero-fills the table for M == 0 — a runtime call — unless another check stops it)
    assert any(s.get(m) == 0 for s in sets) and any(s.get(m, 0) < 0 for s in sets)
    assert sum(len(s) >= 2 for s in sets) >= 1  # two checks fail at once: the precedence
    assert any(c["what"] == f"null {k}" and c["set"] == {k: 0} and c["status"] == make.INVALID for c in rows for k in c["set"])
    if "pts.origins" in make.ENTRIES[entry][1]:
        for k in ("pts.origins", "pts.directions", "pts.t_bins"):
            assert {k: 0} in sets
        assert {"pts.samples_per_ray": 0} in sets and {"pts.samples_per_ray": -48} in sets and {"M": 100} in sets
        assert {"grid.log2_table_size": 0} in sets and {"grid.log2_table_size": 29} in sets
        assert any(s.get("grid.num_levels") == 0 for s in sets) and any(s.get("grid.num_levels") == make.MAX_LEVELS + 1 for s in sets)
        assert {"transform": -1} in sets and {"transform": 3} in sets
    if entry in ("nsamd_field_normals", "nsamd_field_mlp_bwd_scatter_phase"):
        assert {"grid.num_levels": 8} in sets
    if entry == "nsamd_field_mlp_bwd_scatter_phase":
        assert {c["set"]["phase"] for c in rows if list(c["set"]) == ["phase"]} >= {0, 3, 5, 8}


@pytest.mark.parametrize("case", CASES, ids=[f"{i}_{c['entry'][6:]}_{c['what'].replace(' ', '_')}" for i, c in enumerate(CASES)])
def test_entry_point_returns_the_recorded_status(case):
    from nerfstudio_amd import _native as N

    assert make.call(N.load(), case["entry"], case["set"]) == case["status"]
