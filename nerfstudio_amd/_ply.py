"""The binary little-endian PLY both exporters write (pointcloud.PointCloud.write_ply, export.write_mesh_ply)."""
import numpy as np
import torch


def floats(names, t):
    """The columns of `t` `[n, len(names)]` as float properties."""
    return [(name, "<f4", column) for name, column in zip(names, t.detach().float().cpu().numpy().T)]


def colors(t):
    """red green blue uchar = colors * 255 truncated, the product formed in float64 as the reference forms it from its float64
    colours (scripts/exporter.py:183): a colour outside [0, 1] saturates, NaN writes 0."""
    levels = torch.nan_to_num(t.detach().double() * 255, nan=0.0).clamp(0, 255).to(torch.uint8).cpu().numpy()
    return [(name, "u1", column) for name, column in zip(("red", "green", "blue"), levels.T)]


def write(path, properties, faces=None) -> None:
    """properties: the vertex element's (name, "<f4" or "u1", column `[n]` or one value for every row), in file order; faces: `[T,3]`
    int32 for a face element `list uchar int vertex_indices` behind it, or None for no such element."""
    n = len(properties[0][2])
    vertex = np.empty(n, dtype=np.dtype([(name, t) for name, t, _ in properties]))
    for name, _, column in properties:
        vertex[name] = column
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    header += [f"property {'float' if t == '<f4' else 'uchar'} {name}" for name, t, _ in properties]
    face = np.empty(0 if faces is None else len(faces), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    if faces is not None:
        face["n"], face["i"] = 3, faces
        header += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(vertex.tobytes())
        f.write(face.tobytes())
