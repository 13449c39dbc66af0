/*
 * nsamd_mesh.h — the part of libnsamd.so's C ABI that turns a fused TSDF volume into a triangle mesh (ns-export tsdf after
 * nsamd_tsdf_integrate): what TSDF.get_mesh (exporter/tsdf_utils.py:115-136) does with skimage.measure.marching_cubes on a
 * host copy of the volume. Conventions as in nsamd.h: device pointers, dense row-major tensors, a small POD struct passed by
 * value, a hipStream_t; 0 (NSAMD_OK) or a negative nsamd_status, nothing launched on error, no allocation, no
 * synchronisation. Paths are relative to the reference's nerfstudio/ package.
 *
 * The algorithm RESTATES marching cubes at level 0 from its definition: skimage itself was not available to compare against,
 * neither its triangle order nor its vertex normals. The triangle table is generated (scripts/gen_mesh_table.py ->
 * csrc/mesh_table.h); the float64 restatement in tests/mesh_reference.py is this project's definition of the mesh.
 *
 * values [X,Y,Z] fp32 are used as clamp(v, -1, 1) (tsdf_utils.py:121; fmax/fmin: a NaN reads as -1). No mask on the weights,
 * as the reference applies none: unobserved voxels hold -1 and the surface at their border is part of the mesh.
 *   Signs: a corner is NEGATIVE when v < 0 (-0.0 and 0 are not). The cell (i,j,k), i < X-1, j < Y-1, k < Z-1, has corners
 *     c = dx + 2 dy + 4 dz; bit c of its case is set where the corner is negative. Cases 0 and 255 emit nothing.
 *   Vertices: one per crossed lattice edge, owned by the edge's lower voxel p and its axis a. t = v0 / (v0 - v1) in fp32 on the
 *     clamped values, index position p + t e_a, world position origin + index * voxel_size (a multiply, then an add).
 *     Ordered by the owner's linear index (x Y + y) Z + z, then by axis x, y, z.
 *   Faces: int32 [T,3] indices into the vertex array, ordered by the cell's linear index, then by table order. Triangles wind
 *     so that their right-hand normal points toward INCREASING values: out of the surface, into free space.
 *   Degenerate triangles (the reference passes allow_degenerate=False): a vertex SNAPS to a lattice corner when its fp32 t is
 *     exactly 0 (the lower corner) or exactly 1 (the upper one); a triangle with two vertices snapped to the same corner is not
 *     emitted. The count and the emit pass evaluate this one predicate from the same function. Vertices left unreferenced
 *     STAY in the vertex array. (Two vertices with a tiny non-zero t can still round to the same fp32 position.)
 *   Normals: the central-difference gradient of the clamped volume at the edge's two lattice points (one-sided on the volume's
 *     border), each axis divided by its voxel size, blended g0 (1 - t) + g1 t and normalised; a zero gradient gives (0,0,0).
 *     They point toward increasing values, consistent with the winding. ONE KNOWN DEPARTURE from the reference, which passes
 *     no `spacing` to skimage: its normals are in index space even with anisotropic voxels, these are in world space.
 *   Colours: colors[rint(index position)], ties to even (np.round, tsdf_utils.py:128-129), clamped into the volume.
 */
#ifndef NSAMD_MESH_H
#define NSAMD_MESH_H

#include "nsamd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSAMD_MESH_BLOCK 256 /* voxels per workgroup of both entry points */
/* bytes of `scratch` for a volume of n voxels: the totals, two 32-bit words per workgroup, one per voxel (8-byte aligned) */
#define NSAMD_MESH_SCRATCH_BYTES(n) \
  (16 + 8 * (((int64_t)(n) + NSAMD_MESH_BLOCK - 1) / NSAMD_MESH_BLOCK) + 4 * (int64_t)(n))

typedef struct nsamd_mesh_volume {
  float origin[3];     /* world position of voxel (0,0,0) */
  float voxel_size[3]; /* > 0                             */
  int32_t dims[3];     /* X, Y, Z; >= 0                   */
} nsamd_mesh_volume;

/* ------------------------------------------------------------------------------------------------------------
 * Count. One lane per voxel, z fastest: its owned crossed edges (0-3) and its cell's emitted triangles (0-5), scanned inside
 * the workgroup; a one-workgroup launch then scans the workgroups' sums. scratch receives what the emit pass needs: per voxel
 * one word (the voxel's vertex and triangle rank inside its workgroup and its edge mask), per workgroup the number of
 * vertices and of triangles before it, and the totals. totals [2] int64, on the device: the number of vertices and of
 * triangles — the host reads it once to size the outputs, the only synchronisation of an export.
 * No atomics, no waiting between workgroups: the same bits run to run. The triangle table (4 KiB) is staged in LDS by the
 * workgroups that meet a surface. A volume with a dimension below 2 has totals {0, 0}; more than 2^31 - 1 voxels:
 * NSAMD_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_mesh_count(nsamd_mesh_volume vol, const float* values, void* scratch, int64_t* totals, nsamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Emit, after nsamd_mesh_count on the same vol, values and scratch: vertices, normals, vertex_colors [V,3] fp32 and
 * faces [T,3] int32 at the scanned offsets (a wavefront's compacted rows are contiguous); colors [X,Y,Z,3]. A cell finds the
 * id of a vertex on one of its edges from the word of that edge's owner voxel, which may lie in another workgroup's range.
 * V and T are the totals the count pass gave. A V or T outside [0, 3 n] / [0, 5 n] is NSAMD_ERR_INVALID_ARG, one above
 * 2^31 - 1 NSAMD_ERR_UNSUPPORTED (faces are int32); a pair that differs from the totals in scratch writes NOTHING (the
 * comparison is made on the device: the library does not synchronise), and no row at or past V or T is ever written.
 * V == 0 and T == 0 is a no-op.
 * ------------------------------------------------------------------------------------------------------------ */
int nsamd_mesh_emit(nsamd_mesh_volume vol, const float* values, const float* colors, const void* scratch, int64_t V, int64_t T,
                    float* vertices, float* normals, float* vertex_colors, int32_t* faces, nsamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NSAMD_MESH_H */
