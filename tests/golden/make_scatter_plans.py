#!/usr/bin/env python3
"""Records what the table-gradient scatter's workspace queries return, from the built library (host code only, no GPU):

    python tests/golden/make_scatter_plans.py      ->  tests/golden/scatter_plans.json

Per case: the grid (levels, log2 table size, the fp32 scalings as passed), M, and
    words        nsamd_hashgrid_encode_bwd_workspace(grid, M, write_only=0)
    words_set    nsamd_hashgrid_encode_bwd_workspace(grid, M, write_only=1)
    state        nsamd_hashgrid_encode_bwd_workspace_state(grid, M)
    producer     nsamd_field_mlp_bwd_scatter_workspace(grid, M, &producer_state)
    producer_state

Cases: the benchmark's three grids (main table, the two proposal tables) at the benchmark's three point counts, then
off-shape ones: one point, point counts that are no multiple of 1024, tables small enough for the tile size to be clamped
to the table (and to the 256-entry minimum), tables large enough to exceed the tile-count caps (0 words), M = 0.
tests/test_scatter_plans.py asserts exact equality: the plans (tile geometry, queue capacities, workspace layout) are
part of what a caller allocates, and a change to them has to be a decision.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from nerfstudio_amd import _native as N  # noqa: E402
from nerfstudio_amd import functional as F  # noqa: E402

GRIDS = {"main": (16, 16, 2048, 19), "prop0": (5, 16, 128, 17), "prop1": (5, 16, 256, 17)}
BENCH_M = (1048576, 393216, 196608)
OFF_SHAPE = [
    ((16, 16, 2048, 19), 1), ((16, 16, 2048, 19), 1000), ((16, 16, 2048, 19), 196608 + 333), ((5, 16, 128, 17), 1),
    ((5, 16, 256, 17), 393216 - 1), ((16, 16, 2048, 19), 0),
    ((5, 16, 128, 6), 4096), ((5, 16, 128, 9), 12345), ((5, 16, 256, 12), 65536), ((16, 16, 512, 8), 50000),
    ((16, 16, 2048, 14), 196608), ((7, 16, 256, 12), 2049), ((1, 16, 16, 10), 777),
    ((16, 16, 2048, 20), 196608), ((16, 16, 2048, 21), 196608), ((16, 16, 4096, 24), 196608), ((8, 16, 1024, 22), 4096),
    ((16, 16, 2048, 19), 4194304 + 5),
]


def query(spec_args, M):
    lib = N.load()
    spec = F.HashGridSpec(*spec_args)
    scalings = spec.scalings().tolist()
    g = N.make_grid(spec.num_levels, spec.log2_hashmap_size, scalings)
    state = C.c_int64(-1)
    producer = int(lib.nsamd_field_mlp_bwd_scatter_workspace(g, M, C.byref(state)))
    return {
        "num_levels": spec.num_levels, "log2_table_size": spec.log2_hashmap_size, "scalings": scalings, "M": M,
        "words": int(lib.nsamd_hashgrid_encode_bwd_workspace(g, M, 0)),
        "words_set": int(lib.nsamd_hashgrid_encode_bwd_workspace(g, M, 1)),
        "state": int(lib.nsamd_hashgrid_encode_bwd_workspace_state(g, M)),
        "producer": producer,
        "producer_state": int(state.value),  # -1: not written (the query returned 0)
    }


def main():
    cases = [query(g, M) for g in GRIDS.values() for M in BENCH_M] + [query(g, M) for g, M in OFF_SHAPE]
    with open(os.path.join(HERE, "scatter_plans.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    for c in cases:
        print({k: v for k, v in c.items() if k != "scalings"})


if __name__ == "__main__":
    main()
