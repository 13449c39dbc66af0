// TEST INFRASTRUCTURE (tests/test_lens_cpu.py): compiles the per-ray arithmetic of the lens ray generator
// (nerfstudio_amd/csrc/lens.h: undistortion, local directions by camera type and the tail it shares with the pinhole kernels) with
// the HOST compiler, so that `pytest -m "not gpu"` can pin it to the reference's fixture without a GPU. Nothing in the product
// loads this library; the kernels run these functions on the device.
#include <math.h>
#include <stdint.h>

#include "../../nerfstudio_amd/csrc/lens.h"

using namespace nsamd;

extern "C" {

// the loop of raygen_lens_kernel (csrc/misc.hip): ray i = (camera, row, col), pixel centres at +0.5
void hc_raygen_lens(const int64_t* ray_indices, const float* c2w, const float* fx, const float* fy, const float* cx,
                    const float* cy, const int32_t* camera_type, const float* distortion /* [C,6] or null */, int64_t num_rays,
                    float* origins, float* directions, float* pixel_area, float* directions_norm) {
  for (int64_t i = 0; i < num_rays; ++i) {
    const int64_t cam = ray_indices[3 * i + 0];
    const float y = (float)ray_indices[3 * i + 1] + 0.5f;
    const float x = (float)ray_indices[3 * i + 2] + 0.5f;
    raygen_lens_one(x, y, fx[cam], fy[cam], cx[cam], cy[cam], camera_type[cam], distortion ? distortion + 6 * cam : nullptr,
                    c2w + cam * 12, origins + 3 * i, directions + 3 * i, pixel_area + i, directions_norm + i);
  }
}

// lens_undistort on n coordinates xy [n,2] with ONE parameter set k[6], whatever its values (no all-zero shortcut)
void hc_lens_undistort(const float* xy, int64_t n, const float* k, float* out /* [n,2] */) {
  for (int64_t i = 0; i < n; ++i) lens_undistort(xy[2 * i], xy[2 * i + 1], k, out + 2 * i, out + 2 * i + 1);
}

void hc_lens_local_direction(int type, const float* uv, int64_t n, float* out /* [n,3] */) {
  for (int64_t i = 0; i < n; ++i) lens_local_direction(type, uv[2 * i], uv[2 * i + 1], out + 3 * i);
}

int hc_lens_has_distortion(const float* k) { return lens_has_distortion(k) ? 1 : 0; }

}  // extern "C"
