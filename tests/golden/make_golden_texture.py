#!/usr/bin/env python3
"""Golden fixture for the texture export — written by THE REFERENCE ITSELF (read-only import of the reference's
exporter/texture_utils.py: unwrap_mesh_per_uv_triangle and the ray-length line of export_textured_mesh, torch, CPU, fp32).
Authoring container only, with the reference's checkout on the path given by NERFSTUDIO_SRC:

    NERFSTUDIO_SRC=<nerfstudio checkout> python tests/golden/make_golden_texture.py      ->  tests/golden/texture.npz

texture_utils imports mediapy, xatlas, jaxtyping, the ray bundle, exporter_utils (pymeshlab) and the pipelines at module level;
none of them is touched by the two pieces driven here, so stand-ins go into sys.modules first.

Meshes: texture_reference.soup(F) for (F, P) = (1,2), (2,2), (7,4), (37,4) — smooth unit normals, every blend (the extrapolated
ones of the texels past the last face included) of norm >= 0.1, asserted below. Per mesh `m<F>_<P>_`:
    vertices, normals, faces                               the inputs
    texture_coordinates [F,3,2], origins, directions [H,W,3]   what the reference's function returned (before the ray offset)
    raylen                                                 2 * mean |v[f1] - v[f0]|, the reference's fp32 line
    ref_vs_f64_texture_coordinates / _origins / _directions / _raylen
                                                           the reference's own max deviation from the float64 restatement
                                                           (tests/texture_reference.py): its fp32 error, which the tests
                                                           allow the REFERENCE, not the kernel
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_refstubs"))
if os.environ.get("NERFSTUDIO_SRC"):
    sys.path.insert(1, os.environ["NERFSTUDIO_SRC"])
sys.path.insert(2, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import texture_reference as tx  # noqa: E402

CASES = ((1, 2), (2, 2), (7, 4), (37, 4))


def _stub(name, **names):
    m = types.ModuleType(name)
    for k, v in names.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_reference():
    _stub("mediapy")
    _stub("xatlas")
    _stub("nerfstudio.cameras.rays", RayBundle=object)
    _stub("nerfstudio.exporter.exporter_utils", Mesh=object)
    _stub("nerfstudio.pipelines.base_pipeline", Pipeline=object)
    _stub("nerfstudio.utils.rich_utils", CONSOLE=None, get_progress=None)
    from nerfstudio.exporter import texture_utils

    return texture_utils


def main():
    texture_utils = import_reference()
    out = {}
    for F, P in CASES:
        vertices, normals, faces = tx.soup(F)
        tc, origins, directions = texture_utils.unwrap_mesh_per_uv_triangle(
            torch.from_numpy(vertices), torch.from_numpy(faces).long(), torch.from_numpy(normals), P)
        face_vertices = torch.from_numpy(vertices)[torch.from_numpy(faces).long()]
        raylen = 2.0 * torch.mean(torch.norm(face_vertices[:, 1, :] - face_vertices[:, 0, :], dim=-1)).float()  # :378
        sw, sh, W, H = tx.layout(F, P)
        assert tuple(origins.shape) == tuple(directions.shape) == (H, W, 3) and tuple(tc.shape) == (F, 3, 2)
        r = tx.texel_rays(vertices, normals, faces, P, 0.0)
        assert r["blend_norm"].min() >= 0.1, (F, P, r["blend_norm"].min())
        k = f"m{F}_{P}_"
        out[k + "vertices"], out[k + "normals"], out[k + "faces"] = vertices, normals, faces
        out[k + "texture_coordinates"] = tc.numpy().astype(np.float32)
        out[k + "origins"], out[k + "directions"] = origins.numpy(), directions.numpy()
        out[k + "raylen"] = np.float32(raylen.item())
        dev = lambda a, b: np.float64(np.abs(np.asarray(a, np.float64) - b).max())  # noqa: E731
        out[k + "ref_vs_f64_texture_coordinates"] = dev(tc.numpy(), tx.texture_coordinates(F, P))
        out[k + "ref_vs_f64_origins"] = dev(origins.numpy().reshape(-1, 3), r["origins"])
        out[k + "ref_vs_f64_directions"] = dev(directions.numpy().reshape(-1, 3), r["directions"])
        out[k + "ref_vs_f64_raylen"] = dev(raylen.item(), tx.raylen(vertices, faces))
        print(f"F={F} P={P}: atlas {W}x{H}, reference vs float64: tc {out[k + 'ref_vs_f64_texture_coordinates']:.2e}, origins "
              f"{out[k + 'ref_vs_f64_origins']:.2e}, directions {out[k + 'ref_vs_f64_directions']:.2e}, raylen "
              f"{out[k + 'ref_vs_f64_raylen']:.2e}; min blend norm {r['blend_norm'].min():.3f}")
    path = os.path.join(HERE, "texture.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
