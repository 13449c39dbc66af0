#!/usr/bin/env python3
"""Records the status code of entry-point calls that the argument checks answer BEFORE any HIP runtime call, from the built
library (host code only, no GPU):

    python tests/golden/make_launch_checks.py      ->  tests/golden/launch_checks.json

(NSAMD_LIB=<path> records from another build of the library: the table was recorded from the commit before the checks moved
into csrc/launch.h.) Per case: the entry point, the arguments that differ from the entry point's valid call (`set`), and the
status. Pointers are 0 (NULL) or 1 (a non-null address that is never dereferenced: every case returns from the checks).
tests/test_launch_checks.py replays the table: which code an input gets — and which check wins when two fail — is part of
the ABI's behaviour.

A case belongs here only if the checks answer it: NSAMD_OK, NSAMD_ERR_INVALID_ARG or NSAMD_ERR_UNSUPPORTED. main() refuses
to record NSAMD_ERR_LAUNCH / NSAMD_ERR_NO_DEVICE: such a call got as far as the HIP runtime.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from nerfstudio_amd import _native as N  # noqa: E402

OK, INVALID, UNSUPPORTED = 0, -1, -2
MAX_LEVELS = N.MAX_LEVELS
DUMMY = 0x10000  # never dereferenced

POINTS = {"pts.positions": 0, "pts.origins": 1, "pts.directions": 1, "pts.t_bins": 1, "pts.samples_per_ray": 48}
GRID16 = {"grid.num_levels": 16, "grid.log2_table_size": 19}
GRID5 = {"grid.num_levels": 5, "grid.log2_table_size": 17}
FIELD_MLP = {f"mlp.{k}": 1 for k in ("base_W0", "base_b0", "base_W1", "base_b1", "head_W0", "head_b0", "head_W1", "head_b1",
                                      "head_W2", "head_b2", "appearance")}
FIELD_MLP.update({"mlp.num_images": 100, "mlp.ray_terms": 0, "mlp.ray_inputs": 0})
DENSITY_MLP = {"mlp.W0": 1, "mlp.b0": 1, "mlp.W1": 1, "mlp.b1": 1, "mlp.in_dim": 10, "mlp.hidden": 16}
FIELD_ARGS = {"enc": 1, "selector": 1, "directions": 1, "camera_indices": 1, "appearance_const": 0, "dir_group": 48, "M": 96}
FIELD_BWD = {"ddensity": 1, "drgb": 1, "denc": 1, "workspace": 1, "workspace_floats": 1 << 24}
HASH = {"M": 96, "transform": 1, "table": 1, "denc": 1, "stride_p": 1, "stride_k": 96}

# entry point -> (parameters in ABI order, the valid call). Parameter kinds: a struct name, or a scalar / pointer by its name.
ENTRIES = {
    "nsamd_hashgrid_encode_fwd": (
        ["pts", "M", "transform", "aabb", "table", "grid", "enc", "stride_p", "stride_k", "selector", "stream"],
        {**POINTS, **GRID16, "M": 96, "transform": 1, "table": 1, "enc": 1, "stride_p": 1, "stride_k": 96, "selector": 1}),
    "nsamd_hashgrid_encode_bwd": (
        ["pts", "M", "transform", "aabb", "table", "grid", "denc", "stride_p", "stride_k", "dtable", "dpositions", "workspace",
         "workspace_floats", "stream"],
        {**POINTS, **GRID16, **HASH, "dtable": 1, "dpositions": 0, "workspace": 0, "workspace_floats": 0}),
    "nsamd_hashgrid_encode_bwd_set": (
        ["pts", "M", "transform", "aabb", "table", "grid", "denc", "stride_p", "stride_k", "dtable", "dpositions", "workspace",
         "workspace_floats", "stream"],
        {**POINTS, **GRID16, **HASH, "dtable": 1, "dpositions": 0, "workspace": 0, "workspace_floats": 0}),
    "nsamd_hashgrid_encode_bwd_gated": (
        ["pts", "M", "transform", "aabb", "table", "grid", "denc", "stride_p", "stride_k", "dtable", "workspace",
         "workspace_floats", "gate", "ray_mask", "stream"],
        {**POINTS, **GRID5, **HASH, "dtable": 1, "workspace": 1, "workspace_floats": 1 << 24, "gate": 1, "ray_mask": 0}),
    "nsamd_hashgrid_encode_bwd_rays": (
        ["pts", "M", "transform", "aabb", "table", "grid", "denc", "stride_p", "stride_k", "d_origins", "d_directions",
         "accumulate", "stream"],
        {**POINTS, **GRID16, **HASH, "d_origins": 1, "d_directions": 1, "accumulate": 0}),
    "nsamd_field_normals": (
        ["pts", "M", "transform", "aabb", "table", "grid", "enc", "base_W0", "base_b0", "base_W1", "base_b1", "normals",
         "gradient", "geo", "geo_stride", "geo_offset", "stream"],
        {**POINTS, **GRID16, "M": 96, "transform": 1, "table": 1, "enc": 1, "base_W0": 1, "base_b0": 1, "base_W1": 1,
         "base_b1": 1, "normals": 1, "gradient": 0, "geo": 0, "geo_stride": 0, "geo_offset": 0}),
    "nsamd_density_field_fwd": (
        ["pts", "M", "transform", "aabb", "table", "grid", "dmlp", "enc", "selector", "density", "pre", "stream"],
        {**POINTS, **GRID5, **DENSITY_MLP, "M": 96, "transform": 1, "table": 1, "enc": 0, "selector": 0, "density": 1, "pre": 0}),
    "nsamd_field_mlp_bwd_scatter_phase": (
        ["pts", "transform", "aabb", "grid", "enc", "selector", "directions", "camera_indices", "appearance_const", "dir_group",
         "M", "fmlp", "ddensity", "drgb", "denc", "fgrads", "workspace", "workspace_floats", "dtable", "scatter_workspace",
         "scatter_workspace_floats", "phase", "stream"],
        {**POINTS, **GRID16, **FIELD_MLP, **FIELD_ARGS, **FIELD_BWD, "transform": 1, "denc": 0, "dtable": 1,
         "scatter_workspace": 1, "scatter_workspace_floats": 1 << 24, "phase": 7}),
    "nsamd_field_mlp_fwd": (
        ["enc", "selector", "directions", "camera_indices", "appearance_const", "dir_group", "M", "fmlp", "density", "rgb",
         "stream"],
        {**FIELD_MLP, **FIELD_ARGS, "density": 1, "rgb": 1}),
    "nsamd_field_mlp_bwd": (
        ["enc", "selector", "directions", "camera_indices", "appearance_const", "dir_group", "M", "fmlp", "ddensity", "drgb",
         "denc", "fgrads", "workspace", "workspace_floats", "stream"],
        {**FIELD_MLP, **FIELD_ARGS, **FIELD_BWD}),
    "nsamd_field_ray_terms": (
        ["directions", "camera_indices", "appearance_const", "num_rays", "fmlp", "ray_terms", "ray_inputs", "stream"],
        {**FIELD_MLP, "directions": 1, "camera_indices": 1, "appearance_const": 0, "num_rays": 2, "ray_terms": 1,
         "ray_inputs": 0}),
}

_STRUCTS = {"pts": ("pts", N.Points), "grid": ("grid", N.Grid), "dmlp": ("mlp", N.DensityMlp), "fmlp": ("mlp", N.FieldMlp)}


def _value(ctype, v):
    return (DUMMY if v else None) if ctype is N.vp else v


def build_args(entry, overrides):
    """The ctypes arguments of `entry`: its valid call with `overrides` applied."""
    params, valid = ENTRIES[entry]
    unknown = set(overrides) - set(valid)
    assert not unknown, (entry, unknown)  # (a misspelt name would silently test the valid call)
    values = {**valid, **overrides}
    argtypes = N._SIGNATURES[entry]
    assert len(params) == len(argtypes), entry
    args = []
    for name, ctype in zip(params, argtypes):
        if name in _STRUCTS:
            prefix, cls = _STRUCTS[name]
            assert ctype is cls, (entry, name)
            s = cls()
            for field, ftype in cls._fields_:
                key = f"{prefix}.{field}"
                if key in values:
                    setattr(s, field, _value(ftype, values[key]))
            if cls is N.Grid:
                for level in range(MAX_LEVELS):
                    s.scalings[level] = float(16 << min(level, 7))
            args.append(s)
        elif name == "aabb":
            args.append(N.Aabb((N.f32 * 3)(-1, -1, -1), (N.f32 * 3)(1, 1, 1)))
        elif name == "fgrads":
            args.append(N.FieldMlpGrads())  # all NULL: no gradient is asked for
        elif name == "stream":
            args.append(None)
        else:
            args.append(_value(ctype, values[name]))
    return args


def call(lib, entry, overrides):
    return int(getattr(lib, entry)(*build_args(entry, overrides)))


# ---- the cases ---------------------------------------------------------------------------------------------------------------
POINT_CASES = [  # (what, set): calls that fail check_points
    ("M < 0", {"M": -96}),
    ("null origins", {"pts.origins": 0}),
    ("null directions", {"pts.directions": 0}),
    ("null t_bins", {"pts.t_bins": 0}),
    ("samples_per_ray 0", {"pts.samples_per_ray": 0}),
    ("samples_per_ray < 0", {"pts.samples_per_ray": -48}),
    ("M no multiple of samples_per_ray", {"M": 100}),
]
GRID_CASES = [
    ("log2_table_size 0", {"grid.log2_table_size": 0}),
    ("log2_table_size 29", {"grid.log2_table_size": 29}),
    ("num_levels 0", {"grid.num_levels": 0}),
    ("num_levels MAX + 1", {"grid.num_levels": MAX_LEVELS + 1}),
]
TRANSFORM_CASES = [("transform -1", {"transform": -1}), ("transform 3", {"transform": 3})]
BAD_GRID = {"grid.log2_table_size": 29}


def null_cases(*names):
    return [(f"null {n}", {n: 0}) for n in names]


def field_cases(m="M"):
    mlp = [k for k in FIELD_MLP if k not in ("mlp.appearance", "mlp.num_images", "mlp.ray_terms", "mlp.ray_inputs")]
    return [("dir_group 0", {"dir_group": 0}), ("M above the 32-bit offset bound", {m: (1 << 26) + 32}),
            ("camera indices without an appearance table", {"mlp.appearance": 0}),
            ("camera indices with an empty appearance table", {"mlp.num_images": 0}),
            *null_cases("enc", "directions", *mlp)]


CASES = {
    "nsamd_hashgrid_encode_fwd": [
        ("M == 0", {"M": 0}), *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES, *null_cases("table", "enc"),
        ("explicit positions, no rays", {"pts.positions": 1, "pts.origins": 0, "pts.directions": 0, "pts.t_bins": 0,
                                         "pts.samples_per_ray": 0, "transform": 5}),
        ("M == 0 wins over everything", {"M": 0, "table": 0, "transform": 7, **BAD_GRID}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
        ("points win over a bad grid", {"pts.t_bins": 0, **BAD_GRID}),
        ("a bad grid wins over a null table", {"table": 0, **BAD_GRID}),
    ],
    "nsamd_hashgrid_encode_bwd": [
        ("M == 0", {"M": 0}), *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES, *null_cases("denc"),
        ("neither gradient asked for", {"dtable": 0, "dpositions": 0}),
        ("M == 0 wins over a bad grid", {"M": 0, **BAD_GRID}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
        ("a bad grid wins over a null denc", {"denc": 0, "grid.num_levels": 0}),
    ],
    "nsamd_hashgrid_encode_bwd_set": [
        *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES, *null_cases("denc", "dtable"),
        ("M == 0 still checks the grid (the table is to be written)", {"M": 0, **BAD_GRID}),
        ("M == 0 still checks the transform", {"M": 0, "transform": 3}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
    ],
    "nsamd_hashgrid_encode_bwd_gated": [
        ("M == 0", {"M": 0}), *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES, *null_cases("denc", "gate", "dtable", "workspace"),
        ("a null gate wins over M == 0", {"M": 0, "gate": 0}),
        ("a null gate wins over a bad grid", {"gate": 0, **BAD_GRID}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
    ],
    "nsamd_hashgrid_encode_bwd_rays": [
        ("M == 0", {"M": 0}), *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES,
        *null_cases("table", "denc", "d_origins", "d_directions"),
        ("explicit positions have no rays to credit", {"pts.positions": 1}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
        ("a bad grid wins over explicit positions", {"pts.positions": 1, **BAD_GRID}),
    ],
    "nsamd_field_normals": [
        ("M == 0", {"M": 0}), *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES, ("num_levels 8", {"grid.num_levels": 8}),
        *null_cases("table", "enc", "base_W0", "base_b0", "base_W1", "base_b1"),
        ("M above 2^31", {"M": (1 << 31) + 16}),
        ("geo without room for its 15 columns", {"geo": 1, "geo_stride": 14, "geo_offset": 0}),
        ("geo at a negative offset", {"geo": 1, "geo_stride": 32, "geo_offset": -1}),
        ("no output asked for", {"normals": 0, "gradient": 0, "geo": 0}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
        ("a bad grid wins over M == 0", {"M": 0, **BAD_GRID}),
        ("a bad grid wins over the points", {"pts.origins": 0, "grid.num_levels": 8}),
        ("the points win over the transform", {"M": 100, "transform": 3}),
    ],
    "nsamd_density_field_fwd": [
        ("M == 0", {"M": 0}), *POINT_CASES, ("log2_table_size 0", {"grid.log2_table_size": 0}),
        ("log2_table_size 29", {"grid.log2_table_size": 29}), *TRANSFORM_CASES,
        *null_cases("table", "density", "mlp.W0", "mlp.b0", "mlp.W1", "mlp.b1"),
        ("num_levels 0 against the MLP's width", {"grid.num_levels": 0}),
        ("num_levels MAX + 1 against the MLP's width", {"grid.num_levels": MAX_LEVELS + 1}),
        ("num_levels 0 with a matching width", {"grid.num_levels": 0, "mlp.in_dim": 0}),
        ("num_levels MAX + 1 with a matching width", {"grid.num_levels": MAX_LEVELS + 1, "mlp.in_dim": 2 * MAX_LEVELS + 2}),
        ("a level count without an instantiation", {"grid.num_levels": 7, "mlp.in_dim": 14}),
        ("a hidden width without an instantiation", {"mlp.hidden": 32}),
        ("M == 0 wins over a bad grid", {"M": 0, **BAD_GRID}),
        ("M < 0 wins over a bad grid", {"M": -96, **BAD_GRID}),
        ("the points win over a bad grid", {"pts.samples_per_ray": 0, **BAD_GRID}),
        ("a bad table size wins over the MLP's width", {"mlp.in_dim": 16, **BAD_GRID}),
    ],
    "nsamd_field_mlp_bwd_scatter_phase": [
        ("M == 0", {"M": 0}), *POINT_CASES, *GRID_CASES, *TRANSFORM_CASES, ("num_levels 8", {"grid.num_levels": 8}),
        *[(f"phase {p}", {"phase": p}) for p in (0, 3, 5, 8, -1)],
        *null_cases("dtable", "scatter_workspace", "workspace", "ddensity", "drgb"), *field_cases(),
        ("a bad phase wins over M == 0", {"phase": 3, "M": 0}),
        ("M == 0 wins over a bad grid", {"M": 0, "grid.num_levels": 8}),
        ("the level count wins over M < 0", {"M": -96, "grid.num_levels": 8}),
        ("M < 0 with a bad table size", {"M": -96, **BAD_GRID}),
        ("the route's checks win over the field's", {"dtable": 0, "M": (1 << 26) + 32}),
    ],
    "nsamd_field_mlp_fwd": [
        ("M == 0", {"M": 0}), ("M < 0", {"M": -96}), *field_cases(), *null_cases("density"),
        ("M == 0 wins over null pointers", {"M": 0, "enc": 0, "density": 0}),
        ("M < 0 wins over null pointers", {"M": -96, "enc": 0}),
        ("M above the bound wins over null pointers", {"M": (1 << 26) + 32, "enc": 0}),
    ],
    "nsamd_field_mlp_bwd": [
        ("M == 0", {"M": 0}), ("M < 0", {"M": -96}), *field_cases(), *null_cases("ddensity", "drgb", "denc"),
        ("M == 0 wins over null pointers", {"M": 0, "ddensity": 0}),
        ("M above the bound wins over null pointers", {"M": (1 << 26) + 32, "drgb": 0}),
    ],
    "nsamd_field_ray_terms": [
        ("num_rays == 0", {"num_rays": 0}), ("num_rays < 0", {"num_rays": -1}),
        *null_cases("directions", "ray_terms", "mlp.head_W0", "mlp.head_b0"),
        ("camera indices without an appearance table", {"mlp.appearance": 0}),
        ("camera indices with an empty appearance table", {"mlp.num_images": 0}),
        ("num_rays == 0 wins over null pointers", {"num_rays": 0, "directions": 0}),
        ("num_rays < 0 wins over null pointers", {"num_rays": -1, "ray_terms": 0}),
        ("null pointers win over the appearance table", {"ray_terms": 0, "mlp.appearance": 0}),
    ],
}


def main():
    lib = N.load()
    rows = []
    for entry, cases in CASES.items():
        for what, overrides in cases:
            status = call(lib, entry, overrides)
            if status not in (OK, INVALID, UNSUPPORTED):
                sys.exit(f"{entry} [{what}] returned {status}: the call reached the HIP runtime and does not belong in the table")
            rows.append({"entry": entry, "what": what, "set": overrides, "status": status})
    with open(os.path.join(HERE, "launch_checks.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    for r in rows:
        print(r["status"], r["entry"], "|", r["what"])


if __name__ == "__main__":
    main()
