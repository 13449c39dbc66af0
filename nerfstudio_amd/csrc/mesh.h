// Per-voxel arithmetic of the mesh extraction (gfx950; the host compiler sees it only through tests/hostcheck): marching cubes
// at level 0 over a TSDF volume as include/nsamd_mesh.h defines it, where the reference calls skimage
// (exporter/tsdf_utils.py:115-136). The fp32 operation order is stated HERE, once, for the kernels and the host build of the
// tests; the library is built with -ffp-contract=off. skimage's own vertex normals and triangle order cannot be compared where
// this is tested: tests/mesh_reference.py is the definition.
#pragma once

#include "common.h"
#include "../../include/nsamd_mesh.h"

#if defined(__HIPCC__)
#define NSAMD_MESH_TABLE_STORAGE alignas(16) __constant__
#else
#define NSAMD_MESH_TABLE_STORAGE alignas(16) static
#endif
#include "mesh_table.h"

namespace nsamd {

constexpr int kMeshRow = 16;          // bytes per case of the table: 15 edge numbers, then the number of triangles
constexpr int kMeshTableBytes = 256 * kMeshRow;
constexpr int64_t kMeshMaxVoxels = 0x7fffffffLL;

// ---- argument limits, shared by the entry points and the host build of the tests (no HIP runtime call) --------------------------
// *voxels: X Y Z; *meshable: whether every dimension is at least 2 (else there is no cell and no edge to own)
NSAMD_HD int mesh_volume_check(const nsamd_mesh_volume& vol, int64_t* voxels, bool* meshable) {
  for (int a = 0; a < 3; ++a)
    if (vol.dims[a] < 0 || !(vol.voxel_size[a] > 0.0f) || !(vol.origin[a] == vol.origin[a])) return NSAMD_ERR_INVALID_ARG;
  const int64_t plane = (int64_t)vol.dims[1] * vol.dims[2];  // < 2^62
  if (plane > kMeshMaxVoxels || plane * vol.dims[0] > kMeshMaxVoxels) return NSAMD_ERR_UNSUPPORTED;
  *voxels = plane * vol.dims[0];
  *meshable = vol.dims[0] >= 2 && vol.dims[1] >= 2 && vol.dims[2] >= 2;
  return NSAMD_OK;
}

NSAMD_HD int mesh_emit_check(int64_t voxels, int64_t V, int64_t T) {
  if (V < 0 || T < 0 || V > 3 * voxels || T > 5 * voxels) return NSAMD_ERR_INVALID_ARG;
  return (V > 0x7fffffffLL || T > 0x7fffffffLL) ? NSAMD_ERR_UNSUPPORTED : NSAMD_OK;
}

// ---- scratch: [int64 vertices, int64 triangles][u32 per workgroup: vertices before it][u32: triangles before it][u32 per voxel]
struct MeshScratch {
  int64_t* totals;
  uint32_t* vertex_base;    // during the count pass: the workgroup's own number, turned into the base by the scan
  uint32_t* triangle_base;
  uint32_t* words;
};

NSAMD_HD int64_t mesh_blocks(int64_t voxels) { return (voxels + NSAMD_MESH_BLOCK - 1) / NSAMD_MESH_BLOCK; }

NSAMD_HD MeshScratch mesh_scratch(void* scratch, int64_t voxels) {
  MeshScratch s;
  const int64_t blocks = mesh_blocks(voxels);
  s.totals = reinterpret_cast<int64_t*>(scratch);
  s.vertex_base = reinterpret_cast<uint32_t*>(s.totals + 2);
  s.triangle_base = s.vertex_base + blocks;
  s.words = s.triangle_base + blocks;
  return s;
}

// A voxel's word: bits 0-9 its first vertex's rank inside the workgroup (<= 3 * 255), bits 10-12 its edge mask (bit a: the
// edge along axis a from this voxel is crossed), bits 13-23 its cell's first triangle's rank inside the workgroup (<= 5 * 255).
NSAMD_HD uint32_t mesh_word(uint32_t vertex_rank, uint32_t edge_mask, uint32_t triangle_rank) {
  return vertex_rank | (edge_mask << 10) | (triangle_rank << 13);
}
NSAMD_HD uint32_t mesh_word_vertex_rank(uint32_t w) { return w & 1023u; }
NSAMD_HD uint32_t mesh_word_edge_mask(uint32_t w) { return (w >> 10) & 7u; }
NSAMD_HD uint32_t mesh_word_triangle_rank(uint32_t w) { return w >> 13; }

// ---- signs, edges, the crossing -------------------------------------------------------------------------------------------------
NSAMD_HD float mesh_clamp(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }  // tsdf_utils.py:121
NSAMD_HD bool mesh_negative(float v) { return v < 0.0f; }                    // -0.0 and 0 are not
// crossing of an edge whose ends have different signs: the divisor is the sum of two magnitudes, no cancellation; in [0, 1]
NSAMD_HD float mesh_crossing(float v0, float v1) { return v0 / (v0 - v1); }

// edge e = 4 a + u + 2 v (scripts/gen_mesh_table.py): its axis and the corner c = dx + 2 dy + 4 dz it starts from
NSAMD_HD int mesh_edge_axis(int e) { return e >> 2; }
NSAMD_HD int mesh_edge_start(int e) {
  const int a = e >> 2, u = e & 1, v = (e >> 1) & 1;
  return a == 0 ? ((u << 1) | (v << 2)) : (a == 1 ? (u | (v << 2)) : (u | (v << 1)));
}

// Voxel (i,j,k) = linear index lin: the clamped values of the corners of its cell into v[8] (only those inside the volume are
// loaded), the mask of its owned crossed edges (returned) and its cell's case (*code; 0 when the voxel has no cell).
NSAMD_HD uint32_t mesh_voxel_load(const float* values, const nsamd_mesh_volume& vol, int32_t i, int32_t j, int32_t k, int64_t lin,
                                  float* v, int* code) {
  const int64_t sy = vol.dims[2], sx = (int64_t)vol.dims[1] * vol.dims[2];
  const bool hx = i + 1 < vol.dims[0], hy = j + 1 < vol.dims[1], hz = k + 1 < vol.dims[2];
  v[0] = mesh_clamp(values[lin]);
  const bool n0 = mesh_negative(v[0]);
  uint32_t mask = 0;
  if (hx) v[1] = mesh_clamp(values[lin + sx]), mask |= (mesh_negative(v[1]) != n0) ? 1u : 0u;
  if (hy) v[2] = mesh_clamp(values[lin + sy]), mask |= (mesh_negative(v[2]) != n0) ? 2u : 0u;
  if (hz) v[4] = mesh_clamp(values[lin + 1]), mask |= (mesh_negative(v[4]) != n0) ? 4u : 0u;
  *code = 0;
  if (hx && hy && hz) {
    v[3] = mesh_clamp(values[lin + sx + sy]);
    v[5] = mesh_clamp(values[lin + sx + 1]);
    v[6] = mesh_clamp(values[lin + sy + 1]);
    v[7] = mesh_clamp(values[lin + sx + sy + 1]);
    int c = 0;
    for (int b = 0; b < 8; ++b) c |= mesh_negative(v[b]) ? (1 << b) : 0;
    *code = c;
  }
  return mask;
}

NSAMD_HD bool mesh_case_has_surface(int code) { return code != 0 && code != 255; }

// the corner of the cell (0-7) that the vertex on the crossed edge e snaps to, or -1
NSAMD_HD int mesh_snap_corner(const float* v, int e) {
  const int s = mesh_edge_start(e), t = s | (1 << mesh_edge_axis(e));
  const float x = mesh_crossing(v[s], v[t]);
  return x == 0.0f ? s : (x == 1.0f ? t : -1);
}

// THE predicate of both passes: bit n set when triangle n of the case's row is emitted — not two vertices snapped to one corner
NSAMD_HD uint32_t mesh_triangle_mask(const float* v, const unsigned char* row) {
  const int n = row[kMeshRow - 1];
  uint32_t mask = 0;
  for (int t = 0; t < n; ++t) {
    const int a = mesh_snap_corner(v, row[3 * t]), b = mesh_snap_corner(v, row[3 * t + 1]), c = mesh_snap_corner(v, row[3 * t + 2]);
    const bool degenerate = (a >= 0 && (a == b || a == c)) || (b >= 0 && b == c);
    mask |= degenerate ? 0u : (1u << t);
  }
  return mask;
}

// ---- a vertex -------------------------------------------------------------------------------------------------------------------
// World-space gradient of the clamped volume at lattice point q: central differences, one-sided on the border (every dimension
// is at least 2), each axis divided by its voxel size.
NSAMD_HD void mesh_gradient(const float* values, const nsamd_mesh_volume& vol, const int32_t* q, int64_t lin, float* g) {
  const int64_t stride[3] = {(int64_t)vol.dims[1] * vol.dims[2], vol.dims[2], 1};
  for (int b = 0; b < 3; ++b) {
    const bool lower = q[b] > 0, upper = q[b] + 1 < vol.dims[b];
    const float lo = mesh_clamp(values[lower ? lin - stride[b] : lin]), hi = mesh_clamp(values[upper ? lin + stride[b] : lin]);
    const float d = (lower && upper) ? (hi - lo) / 2.0f : hi - lo;
    g[b] = d / vol.voxel_size[b];
  }
}

// The vertex on the crossed edge along axis a from voxel p (linear index lin), whose ends hold the clamped v0 and v1: row `at`
// of the three outputs.
NSAMD_HD void mesh_emit_vertex(const float* values, const float* colors, const nsamd_mesh_volume& vol, const int32_t* p, int64_t lin,
                               int a, float v0, float v1, int64_t at, float* vertices, float* normals, float* vertex_colors) {
  const int64_t stride[3] = {(int64_t)vol.dims[1] * vol.dims[2], vol.dims[2], 1};
  const float t = mesh_crossing(v0, v1);
  float index[3] = {(float)p[0], (float)p[1], (float)p[2]};
  index[a] = index[a] + t;
  for (int b = 0; b < 3; ++b) vertices[3 * at + b] = vol.origin[b] + index[b] * vol.voxel_size[b];

  int32_t q[3] = {p[0], p[1], p[2]};
  float g0[3], g1[3], n[3];
  mesh_gradient(values, vol, q, lin, g0);
  q[a] += 1;
  mesh_gradient(values, vol, q, lin + stride[a], g1);
  for (int b = 0; b < 3; ++b) n[b] = g0[b] * (1.0f - t) + g1[b] * t;
  const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  for (int b = 0; b < 3; ++b) normals[3 * at + b] = len > 0.0f ? n[b] / len : 0.0f;

  const float r = nearbyintf(index[a]);  // ties to even; p[a] <= r <= p[a] + 1 < dims[a]
  int32_t ca = (int32_t)r;
  ca = ca < 0 ? 0 : (ca > vol.dims[a] - 1 ? vol.dims[a] - 1 : ca);
  const int64_t voxel = lin + (int64_t)(ca - p[a]) * stride[a];
  for (int b = 0; b < 3; ++b) vertex_colors[3 * at + b] = colors[3 * voxel + b];
}

// Id of the vertex on edge e of the cell at linear index lin, from the word of the edge's owner voxel.
NSAMD_HD int64_t mesh_edge_vertex(const MeshScratch& s, const nsamd_mesh_volume& vol, int64_t lin, int e) {
  const int c = mesh_edge_start(e), a = mesh_edge_axis(e);
  const int64_t owner = lin + (c & 1) * ((int64_t)vol.dims[1] * vol.dims[2]) + ((c >> 1) & 1) * (int64_t)vol.dims[2] + (c >> 2);
  const uint32_t w = s.words[owner];
  const uint32_t before = (uint32_t)__builtin_popcount(mesh_word_edge_mask(w) & ((1u << a) - 1u));
  return (int64_t)s.vertex_base[owner / NSAMD_MESH_BLOCK] + mesh_word_vertex_rank(w) + before;
}

}  // namespace nsamd
