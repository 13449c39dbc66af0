"""Generates nerfstudio_amd/csrc/mesh_table.h, the marching-cubes triangle table of the mesh export (include/nsamd_mesh.h).

    python scripts/gen_mesh_table.py > nerfstudio_amd/csrc/mesh_table.h

The table is DERIVED, not typed in; tests/test_mesh_cpu.py runs this module and compares its output with the committed header,
and tests/mesh_reference.py takes the table from here.

Numbering. Corner c = dx + 2 dy + 4 dz of a cell. Edge e = 4 a + u + 2 v runs along axis a from the corner whose two other
coordinates (in increasing axis order) are (u, v): edges 0-3 along x at (dy, dz) = (0,0) (1,0) (0,1) (1,1), 4-7 along y at
(dx, dz), 8-11 along z at (dx, dy). Bit c of a case is set where corner c is NEGATIVE.

Rule. Every face of the cube is walked counter-clockwise as seen from outside. Each maximal run of negative corners on that
walk (a face that is neither all negative nor all non-negative has one run, or two runs of one corner each: the ambiguous
face) gives one segment, from the edge on which the walk enters the run to the edge on which it leaves it. That depends on the
face's four signs alone, so the two cells that share a face draw the same segments on it. An edge of the cube lies in two
faces, which walk it in opposite directions: every crossed edge is the head of one segment and the tail of another, and the
segments chain into closed loops. A loop is rotated to start at its lowest-numbered edge and fan-triangulated from there; the
loops of a case are ordered by that edge. Triangles wind so that their right-hand normal points toward the non-negative side
(toward increasing values: out of the surface).
"""
import sys

import numpy as np

ROW = 16  # bytes per case: 15 edge numbers (5 triangles), then the number of triangles
UNUSED = 255


def corner_xyz(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_corners(e):
    """(start corner, end corner, axis): the end is the start plus one along the axis"""
    a, u, v = e // 4, e % 2, (e % 4) // 2
    others = [b for b in range(3) if b != a]
    start = (u << others[0]) | (v << others[1])
    return start, start | (1 << a), a


EDGE_OF = {}
for _e in range(12):
    _s, _t, _ = edge_corners(_e)
    EDGE_OF[(_s, _t)] = EDGE_OF[(_t, _s)] = _e


def faces():
    """the six faces as corner cycles, counter-clockwise seen from outside"""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3  # e_b x e_c = e_a
        for side in (0, 1):
            cycle = [(side << a) | (u << b) | (v << c) for u, v in ((0, 0), (1, 0), (1, 1), (0, 1))]
            if side == 0:
                cycle.reverse()
            p = [np.array(corner_xyz(k), float) for k in cycle]
            normal = np.cross(p[1] - p[0], p[2] - p[1])
            assert normal[a] == (1 if side else -1) and abs(normal).sum() == 1
            out.append(cycle)
    return out


FACES = faces()


def case_segments(case):
    """directed segments (from edge, to edge) of a case, face by face"""
    neg = [(case >> c) & 1 for c in range(8)]
    segs = []
    for cycle in FACES:
        s = [neg[c] for c in cycle]
        if sum(s) in (0, 4):
            continue
        for i in range(4):
            if s[i] and not s[i - 1]:  # the walk enters a run of negative corners at cycle[i]
                j = i
                while s[(j + 1) % 4]:
                    j += 1
                segs.append((EDGE_OF[(cycle[i - 1], cycle[i])], EDGE_OF[(cycle[j % 4], cycle[(j + 1) % 4])]))
    return segs


def case_loops(case):
    segs = case_segments(case)
    nxt = dict(segs)
    crossed = sorted(e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1)
    assert sorted(nxt) == sorted(nxt.values()) == crossed and len(segs) == len(crossed), case
    loops, seen = [], set()
    for e in crossed:
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def _flip():
    """case 1 (corner 0 negative): the triangle over edges 0, 4, 8 must face (+, +, +)"""
    (loop,) = case_loops(1)
    mid = [np.array([0.5 * (np.array(corner_xyz(edge_corners(e)[0])) + np.array(corner_xyz(edge_corners(e)[1])))]).reshape(3)
           for e in loop]
    return float(np.cross(mid[1] - mid[0], mid[2] - mid[0]).sum()) < 0


FLIP = _flip()


def triangle_table():
    """256 lists of (e0, e1, e2)"""
    table = []
    for case in range(256):
        tris = []
        for loop in case_loops(case):
            for i in range(1, len(loop) - 1):
                tris.append((loop[0], loop[i + 1], loop[i]) if FLIP else (loop[0], loop[i], loop[i + 1]))
        table.append(tris)
    return table


def table_bytes():
    """[256, 16] uint8: the committed layout"""
    rows = np.full((256, ROW), UNUSED, np.uint8)
    for case, tris in enumerate(triangle_table()):
        assert len(tris) <= 5
        rows[case, :3 * len(tris)] = np.array(tris, np.uint8).reshape(-1)
        rows[case, ROW - 1] = len(tris)
    return rows


def header_text():
    rows = table_bytes()
    lines = ["// GENERATED by scripts/gen_mesh_table.py — do not edit; tests/test_mesh_cpu.py compares it with the generator's output.",
             "// Marching-cubes triangles per 8-bit case (bit c set: corner c = dx + 2 dy + 4 dz is negative). A row is 16 bytes: up to",
             "// 5 triangles of 3 edge numbers (edge 4 a + u + 2 v: along axis a from the corner at (u, v) of the other two axes), 255",
             "// where unused, and in byte 15 the number of triangles. %d triangles in all." % int(rows[:, ROW - 1].sum()),
             "#pragma once",
             "",
             "NSAMD_MESH_TABLE_STORAGE const unsigned char kMeshTriangleTable[256 * 16] = {"]
    for case in range(256):
        lines.append("    " + ", ".join("%3d" % b for b in rows[case]) + ",  // %3d" % case)
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    sys.stdout.write(header_text())
