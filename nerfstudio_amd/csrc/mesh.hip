// Mesh extraction from a TSDF volume (include/nsamd_mesh.h): nsamd_mesh_count / nsamd_mesh_emit. What the reference does with
// skimage's marching cubes on a host copy of the volume (exporter/tsdf_utils.py:115-136) is an ordered, data-dependent stream
// compaction over the voxels here, in the three launches that block_scan.h describes and serves: per-workgroup counts, a
// one-workgroup scan, writes — every placement a sum of counts, no atomics, no workgroup waiting for another. Both passes
// are bandwidth-bound: the values are read once from memory per pass (the seven neighbour reads of a lane hit the lines its
// own and the neighbouring wavefronts fetch), the per-voxel words are written by the count pass and read by the emit pass.
// The per-voxel arithmetic is mesh.h.
#include "block_scan.h"
#include "launch.h"
#include "mesh.h"

using namespace nsamd;

namespace {

constexpr int kMeshThreads = NSAMD_MESH_BLOCK;  // four wavefronts
constexpr int kMeshWaves = kMeshThreads / 64;
static_assert(kMeshTableBytes == kMeshThreads * 16, "one 16-byte row of the table per thread");

// voxel (i,j,k) of linear index lin, z fastest
__device__ __forceinline__ void mesh_voxel_of(const nsamd_mesh_volume& vol, int64_t lin, int32_t* p) {
  const int64_t plane = (int64_t)vol.dims[1] * vol.dims[2];
  const int64_t i = point_ray(lin, plane);
  const int64_t rest = lin - i * plane;
  const int64_t j = point_ray(rest, vol.dims[2]);
  p[0] = (int32_t)i, p[1] = (int32_t)j, p[2] = (int32_t)(rest - j * vol.dims[2]);
}

// The triangle table into LDS, by the workgroups in which some lane's cell meets a surface (most of a volume's do not). All
// threads of the block call it with their own `surface`; returns whether the table was staged.
__device__ __forceinline__ bool stage_table(bool surface, unsigned char* table) {
  if (!__syncthreads_or(surface ? 1 : 0)) return false;
  reinterpret_cast<uint4*>(table)[threadIdx.x] = reinterpret_cast<const uint4*>(kMeshTriangleTable)[threadIdx.x];
  __syncthreads();
  return true;
}

// One lane per voxel. Vertices (0-3) and triangles (0-5) of the lane as one packed 32-bit count — a workgroup's sums, 768 and
// 1280 at most, stay inside their 16-bit halves — scanned over the workgroup in one call (block_scan.h). Lanes past the volume
// count nothing and stay active for the scan.
__global__ __launch_bounds__(kMeshThreads) void mesh_count_kernel(nsamd_mesh_volume vol, int64_t voxels,
                                                                  const float* __restrict__ values, void* scratch) {
  __shared__ __attribute__((aligned(16))) unsigned char table[kMeshTableBytes];
  const MeshScratch s = mesh_scratch(scratch, voxels);
  const int64_t lin = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  const bool active = lin < voxels;
  float v[8];
  int code = 0;
  uint32_t edge_mask = 0, triangle_mask = 0;
  if (active) {
    int32_t p[3];
    mesh_voxel_of(vol, lin, p);
    edge_mask = mesh_voxel_load(values, vol, p[0], p[1], p[2], lin, v, &code);
  }
  const bool surface = mesh_case_has_surface(code);
  if (stage_table(surface, table) && surface) triangle_mask = mesh_triangle_mask(v, table + kMeshRow * code);

  const uint32_t mine = (uint32_t)__popc(edge_mask) | ((uint32_t)__popc(triangle_mask) << 16);
  uint32_t exclusive, sum;
  block_scan_exclusive_u32<kMeshWaves>(&mine, &exclusive, &sum);
  if (active) s.words[lin] = mesh_word(exclusive & 0xffffu, edge_mask, exclusive >> 16);
  if (threadIdx.x == 0) {
    s.vertex_base[blockIdx.x] = sum & 0xffffu;
    s.triangle_base[blockIdx.x] = sum >> 16;
  }
}

// ONE workgroup: exclusive scan in place of the workgroups' vertex and triangle counts (the two-channel sweep of block_scan.h);
// the totals into scratch and into totals[2]. A base above 2^32 wraps: the emit entry point refuses such totals.
__global__ __launch_bounds__(kMeshThreads) void mesh_scan_kernel(void* scratch, int64_t voxels, int64_t blocks,
                                                                 int64_t* __restrict__ totals) {
  const MeshScratch s = mesh_scratch(scratch, voxels);
  uint32_t* const counts[2] = {s.vertex_base, s.triangle_base};
  uint64_t sum[2];
  block_sweep_exclusive_u32<kMeshWaves, 2>(counts, blocks, sum);
  if (threadIdx.x != 0) return;
  s.totals[0] = totals[0] = (int64_t)sum[0];
  s.totals[1] = totals[1] = (int64_t)sum[1];
}

// One lane per voxel again: the lane writes the vertices it owns and the triangles of its cell, at its workgroup's base plus
// the rank in its word — consecutive lanes write consecutive rows. Nothing is scanned here. The totals are compared first
// (uniform over the launch), and no row at or past V or T is written even if `values` changed since the count.
__global__ __launch_bounds__(kMeshThreads) void mesh_emit_kernel(nsamd_mesh_volume vol, int64_t voxels,
                                                                 const float* __restrict__ values, const float* __restrict__ colors,
                                                                 const void* scratch, int64_t V, int64_t T,
                                                                 float* __restrict__ vertices, float* __restrict__ normals,
                                                                 float* __restrict__ vertex_colors, int32_t* __restrict__ faces) {
  __shared__ __attribute__((aligned(16))) unsigned char table[kMeshTableBytes];
  const MeshScratch s = mesh_scratch(const_cast<void*>(scratch), voxels);
  if (s.totals[0] != V || s.totals[1] != T) return;
  const int64_t lin = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
  const bool active = lin < voxels;
  float v[8];
  int code = 0;
  int32_t p[3] = {0, 0, 0};
  uint32_t word = 0;
  if (active) {
    mesh_voxel_of(vol, lin, p);
    const uint32_t edge_mask = mesh_voxel_load(values, vol, p[0], p[1], p[2], lin, v, &code);
    word = s.words[lin];
    int64_t at = (int64_t)s.vertex_base[blockIdx.x] + mesh_word_vertex_rank(word);
    for (int a = 0; a < 3; ++a) {
      if (!(edge_mask & (1u << a))) continue;
      if (at < V) mesh_emit_vertex(values, colors, vol, p, lin, a, v[0], v[1 << a], at, vertices, normals, vertex_colors);
      ++at;
    }
  }
  const bool surface = mesh_case_has_surface(code);
  if (!stage_table(surface, table) || !surface) return;
  const unsigned char* row = table + kMeshRow * code;
  const uint32_t triangle_mask = mesh_triangle_mask(v, row);
  int64_t at = (int64_t)s.triangle_base[blockIdx.x] + mesh_word_triangle_rank(word);
  for (int t = 0; t < row[kMeshRow - 1]; ++t) {
    if (!(triangle_mask & (1u << t))) continue;
    if (at < T)
      for (int c = 0; c < 3; ++c) faces[3 * at + c] = (int32_t)mesh_edge_vertex(s, vol, lin, row[3 * t + c]);
    ++at;
  }
}

}  // namespace

extern "C" int nsamd_mesh_count(nsamd_mesh_volume vol, const float* values, void* scratch, int64_t* totals,
                                nsamd_stream_t stream) {
  int64_t voxels = 0;
  bool meshable = false;
  const int sizes = mesh_volume_check(vol, &voxels, &meshable);
  if (sizes != NSAMD_OK) return sizes;
  NSAMD_REQUIRE(scratch != nullptr && totals != nullptr && (values != nullptr || !meshable));
  const int64_t nblocks = meshable ? mesh_blocks(voxels) : 0;  // no cell, no edge: the scan alone writes the zero totals
  unsigned blocks = 0;
  const int status = grid_blocks(nblocks, &blocks);
  if (status != NSAMD_OK) return status;
  hipStream_t s = (hipStream_t)stream;
  if (nblocks > 0) {
    mesh_count_kernel<<<blocks, kMeshThreads, 0, s>>>(vol, voxels, values, scratch);
    NSAMD_CHECK_LAUNCH();
  }
  mesh_scan_kernel<<<1, kMeshThreads, 0, s>>>(scratch, voxels, nblocks, totals);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}

extern "C" int nsamd_mesh_emit(nsamd_mesh_volume vol, const float* values, const float* colors, const void* scratch, int64_t V,
                               int64_t T, float* vertices, float* normals, float* vertex_colors, int32_t* faces,
                               nsamd_stream_t stream) {
  int64_t voxels = 0;
  bool meshable = false;
  const int sizes = mesh_volume_check(vol, &voxels, &meshable);
  if (sizes != NSAMD_OK) return sizes;
  const int counts = mesh_emit_check(meshable ? voxels : 0, V, T);
  if (counts != NSAMD_OK) return counts;
  if (V == 0 && T == 0) return NSAMD_OK;
  NSAMD_REQUIRE(values && colors && scratch && (V == 0 || (vertices && normals && vertex_colors)) && (T == 0 || faces));
  unsigned blocks = 0;
  const int status = grid_blocks(mesh_blocks(voxels), &blocks);
  if (status != NSAMD_OK) return status;
  mesh_emit_kernel<<<blocks, kMeshThreads, 0, (hipStream_t)stream>>>(vol, voxels, values, colors, scratch, V, T, vertices, normals,
                                                                     vertex_colors, faces);
  NSAMD_CHECK_LAUNCH();
  return NSAMD_OK;
}
