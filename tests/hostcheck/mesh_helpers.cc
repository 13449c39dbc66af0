// Host build of nerfstudio_amd/csrc/mesh.h for tests/test_mesh_cpu.py (and tests/hostcheck/mesh_main.cc): the per-voxel
// arithmetic of the mesh entry points, looped the way the kernels compose it — workgroups of 256 voxels counted and ranked, the
// workgroups' sums scanned, then every voxel writing its vertices and its cell's triangles at base + rank, a vertex's id read
// from its owner voxel's word. Host memory in place of device memory; the scratch layout and the argument checks are the entry
// points' own (mesh.h). Test infrastructure: the product never loads it.
#include "../../nerfstudio_amd/csrc/mesh.h"

using namespace nsamd;

namespace {

void voxel_of(const nsamd_mesh_volume& vol, int64_t lin, int32_t* p) {
  const int64_t plane = (int64_t)vol.dims[1] * vol.dims[2];
  p[0] = (int32_t)(lin / plane);
  p[1] = (int32_t)((lin % plane) / vol.dims[2]);
  p[2] = (int32_t)(lin % vol.dims[2]);
}

}  // namespace

extern "C" int hc_mesh_count(nsamd_mesh_volume vol, const float* values, void* scratch, int64_t* totals) {
  int64_t voxels = 0;
  bool meshable = false;
  const int sizes = mesh_volume_check(vol, &voxels, &meshable);
  if (sizes != NSAMD_OK) return sizes;
  if (!(scratch != nullptr && totals != nullptr && (values != nullptr || !meshable))) return NSAMD_ERR_INVALID_ARG;
  const MeshScratch s = mesh_scratch(scratch, voxels);
  const int64_t blocks = meshable ? mesh_blocks(voxels) : 0;
  for (int64_t b = 0; b < blocks; ++b) {
    uint32_t nv = 0, nt = 0;
    for (int64_t lin = b * NSAMD_MESH_BLOCK; lin < voxels && lin < (b + 1) * NSAMD_MESH_BLOCK; ++lin) {
      int32_t p[3];
      float v[8];
      int code = 0;
      voxel_of(vol, lin, p);
      const uint32_t edge_mask = mesh_voxel_load(values, vol, p[0], p[1], p[2], lin, v, &code);
      const uint32_t triangle_mask = mesh_case_has_surface(code) ? mesh_triangle_mask(v, kMeshTriangleTable + kMeshRow * code) : 0u;
      s.words[lin] = mesh_word(nv, edge_mask, nt);
      nv += (uint32_t)__builtin_popcount(edge_mask);
      nt += (uint32_t)__builtin_popcount(triangle_mask);
    }
    s.vertex_base[b] = nv;
    s.triangle_base[b] = nt;
  }
  uint64_t carry[2] = {0, 0};
  for (int64_t b = 0; b < blocks; ++b) {
    const uint32_t nv = s.vertex_base[b], nt = s.triangle_base[b];
    s.vertex_base[b] = (uint32_t)carry[0];
    s.triangle_base[b] = (uint32_t)carry[1];
    carry[0] += nv;
    carry[1] += nt;
  }
  s.totals[0] = totals[0] = (int64_t)carry[0];
  s.totals[1] = totals[1] = (int64_t)carry[1];
  return NSAMD_OK;
}

extern "C" int hc_mesh_emit(nsamd_mesh_volume vol, const float* values, const float* colors, const void* scratch, int64_t V,
                            int64_t T, float* vertices, float* normals, float* vertex_colors, int32_t* faces) {
  int64_t voxels = 0;
  bool meshable = false;
  const int sizes = mesh_volume_check(vol, &voxels, &meshable);
  if (sizes != NSAMD_OK) return sizes;
  const int counts = mesh_emit_check(meshable ? voxels : 0, V, T);
  if (counts != NSAMD_OK) return counts;
  if (V == 0 && T == 0) return NSAMD_OK;
  if (!(values && colors && scratch && (V == 0 || (vertices && normals && vertex_colors)) && (T == 0 || faces)))
    return NSAMD_ERR_INVALID_ARG;
  const MeshScratch s = mesh_scratch(const_cast<void*>(scratch), voxels);
  if (s.totals[0] != V || s.totals[1] != T) return NSAMD_OK;  // the kernel writes nothing
  for (int64_t lin = 0; lin < voxels; ++lin) {
    int32_t p[3];
    float v[8];
    int code = 0;
    voxel_of(vol, lin, p);
    const uint32_t edge_mask = mesh_voxel_load(values, vol, p[0], p[1], p[2], lin, v, &code);
    const uint32_t word = s.words[lin];
    int64_t at = (int64_t)s.vertex_base[lin / NSAMD_MESH_BLOCK] + mesh_word_vertex_rank(word);
    for (int a = 0; a < 3; ++a) {
      if (!(edge_mask & (1u << a))) continue;
      if (at < V) mesh_emit_vertex(values, colors, vol, p, lin, a, v[0], v[1 << a], at, vertices, normals, vertex_colors);
      ++at;
    }
    if (!mesh_case_has_surface(code)) continue;
    const unsigned char* row = kMeshTriangleTable + kMeshRow * code;
    const uint32_t triangle_mask = mesh_triangle_mask(v, row);
    at = (int64_t)s.triangle_base[lin / NSAMD_MESH_BLOCK] + mesh_word_triangle_rank(word);
    for (int t = 0; t < row[kMeshRow - 1]; ++t) {
      if (!(triangle_mask & (1u << t))) continue;
      if (at < T)
        for (int c = 0; c < 3; ++c) faces[3 * at + c] = (int32_t)mesh_edge_vertex(s, vol, lin, row[3 * t + c]);
      ++at;
    }
  }
  return NSAMD_OK;
}
