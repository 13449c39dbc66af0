// Backward of ALL proposal levels of an iteration that updates the proposal networks (ProposalNetworkSampler,
// /root/reference/nerfstudio/model_components/ray_samplers.py:590-609 -> RaySamples.get_weights backward, cameras/rays.py:129-152
// -> HashMLPDensityField backward, fields/density_fields.py:94-117 -> HashEncoding backward, field_components/encodings.py:417-458)
// as one entry point: nsamd_proposal_levels_bwd.
//
// Per level the chain is six launches (weights backward with the zero-gradient gate, density-MLP backward, the fixed-order
// reduce of its weight-gradient partials, the scatter's route / apply / finish passes), and every one of them is as long as
// its slowest workgroup's chain of memory round trips, not as its work (profiles/r06_s25_*, r06_s26_*: the run kernel's live
// waves spend 16 - 30 us in two sweeps whether 5 or 900 of 4096 rays carry gradient). The levels share nothing — separate
// networks, tables, gradients, scratch —, so here the SAME stage of two levels is one launch (blockIdx.y / .z selects the
// level, every workgroup runs the unchanged per-level body): twelve launches become six, and two latency chains run side
// by side. Same bits as the per-level entry points, call by call. Whether two calls of a stage can share its launches is the
// stage's own launcher's business (proposal_chain.h, scatter.h); where they cannot, it runs them one after the other.
// (The weights stage runs one call through the same kernel, with one slice; the density and scatter stages have a
// single-call kernel around the same body for that, proposal_chain.h says why.)
#include "launch.h"
#include "proposal_chain.h"
#include "scatter.h"

using namespace nsamd;

static int level_checks(const nsamd_proposal_level_bwd& l) {
  NSAMD_REQUIRE(l.num_rays > 0 && l.samples_per_ray > 0 && l.samples_per_ray <= 1024);
  NSAMD_REQUIRE(l.t_bins && l.density && l.dweights && l.ddensity && l.gate && l.ray_mask);
  NSAMD_REQUIRE(l.enc && l.pre && l.denc && l.dW0 && l.db0 && l.dW1 && l.db1 && l.mlp.W0 && l.mlp.b0 && l.mlp.W1 && l.mlp.b1);
  NSAMD_REQUIRE(l.origins && l.directions && l.table && l.dtable && l.scatter_workspace);
  NSAMD_REQUIRE(l.transform >= 0 && l.transform <= 2);
  NSAMD_REQUIRE(l.grid.num_levels > 0 && l.grid.num_levels <= NSAMD_MAX_LEVELS && 2 * l.grid.num_levels == l.mlp.in_dim);
  if (!table_size_ok(l.grid)) return NSAMD_ERR_UNSUPPORTED;
  return NSAMD_OK;
}

static nsamd_points level_points(const nsamd_proposal_level_bwd& l) {
  nsamd_points p{};
  p.positions = nullptr;
  p.origins = l.origins;
  p.directions = l.directions;
  p.t_bins = l.t_bins;
  p.samples_per_ray = l.samples_per_ray;
  return p;
}

static ScatterCall level_scatter(const nsamd_proposal_level_bwd& l) {
  const int64_t M = l.num_rays * l.samples_per_ray;
  return ScatterCall{level_points(l), M, l.transform, l.aabb, l.grid, l.denc, 1, M, l.dtable, l.scatter_workspace,
                     scatter_plan_in(l.grid, M, false, l.scatter_workspace, l.scatter_workspace_floats), false, l.gate, l.ray_mask};
}

extern "C" int nsamd_proposal_levels_bwd(const nsamd_proposal_level_bwd* levels, int32_t num_levels, int32_t gates_precleared,
                                         nsamd_stream_t stream) {
  NSAMD_REQUIRE(num_levels >= 0 && (num_levels == 0 || levels != nullptr));
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < num_levels; ++i) {
    const int rc = level_checks(levels[i]);
    if (rc) return rc;
  }
  if (!gates_precleared) {
    for (int i = 0; i < num_levels; ++i)
      if (hipMemsetAsync(levels[i].gate, 0, sizeof(uint32_t), st) != hipSuccess) return NSAMD_ERR_LAUNCH;
  }
  for (int i = 0; i < num_levels; i += 2) {
    const int n = i + 1 < num_levels ? 2 : 1;  // levels i, i + 1 stage by stage, or an odd level out alone
    WeightsBwdCall weights[2];
    DensityBwdCall density[2];
    ScatterCall scatter[2];
    for (int j = 0; j < n; ++j) {
      const nsamd_proposal_level_bwd& l = levels[i + j];
      weights[j] = WeightsBwdCall{l.t_bins, l.density, l.dweights, l.num_rays, l.samples_per_ray, l.ddensity, l.gate, l.ray_mask};
      density[j] = DensityBwdCall{l.enc, l.selector, l.pre, l.ddensity, l.num_rays * l.samples_per_ray, l.mlp, l.denc, l.dW0, l.db0,
                                  l.dW1, l.db1, l.mlp_workspace, l.mlp_workspace_floats, l.gate, l.ray_mask, l.samples_per_ray};
      scatter[j] = level_scatter(l);
    }
    int rc = weights_bwd_launch(weights, n, st);        // RaySamples.get_weights backward + gate
    if (!rc) rc = density_bwd_launch(density, n, st);  // density MLP backward + weight-gradient reduce
    if (!rc) rc = scatter_launch(scatter, n, st);      // table scatter: route, apply, finish
    if (rc) return rc;
  }
  return NSAMD_OK;
}
