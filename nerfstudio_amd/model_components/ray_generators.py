"""Ray generator (reference: nerfstudio/model_components/ray_generators.py:26-56)."""
import torch
from torch import Tensor, nn

from .. import functional as F
from ..cameras.rays import RayBundle


class RayGenerator(nn.Module):
    """(camera, row, col) pixel indices -> RayBundle, as one HIP kernel (csrc/misc.hip, csrc/lens.h).

    `cameras` is anything exposing nerfstudio's `Cameras` tensors: `camera_to_worlds [C,3,4]`, `fx, fy, cx, cy [C]`
    or `[C,1]`, and optionally `camera_type [C]` / `[C,1]` and `distortion_params [C,6]` (cameras/cameras.py:88-170).
    Perspective, fisheye and equirectangular cameras (CameraType 1 - 3) with per-camera distortion are covered, mixed freely;
    when every camera is an undistorted perspective one the pinhole kernel runs. Omnidirectional-stereo, VR180, orthophoto and
    fisheye624 cameras are rejected.
    """

    def __init__(self, cameras) -> None:
        super().__init__()
        self.cameras = cameras
        c2w = torch.as_tensor(cameras.camera_to_worlds).float().reshape(-1, 3, 4).clone()
        num_cameras = c2w.shape[0]
        ctype = getattr(cameras, "camera_type", None)
        if ctype is None:
            ctype = torch.ones(num_cameras, dtype=torch.int32)  # CameraType.PERSPECTIVE
        else:
            ctype = torch.as_tensor(ctype).reshape(-1).to(torch.int32).clone()
            if ctype.numel() == 1:
                ctype = ctype.expand(num_cameras).clone()
        F.check_lens_types(ctype)
        dist = getattr(cameras, "distortion_params", None)
        dist = torch.zeros(num_cameras, 6) if dist is None else torch.as_tensor(dist).float().reshape(-1, 6).clone()
        if ctype.numel() != num_cameras or dist.shape[0] != num_cameras:
            raise ValueError("camera_type and distortion_params must have one row per camera")
        # undistorted perspective cameras only: the pinhole kernel (equirectangular cameras are never undistorted)
        self.pinhole = bool((ctype == 1).all()) and not bool((dist != 0).any())
        self.register_buffer("c2w", c2w, persistent=False)
        for name in ("fx", "fy", "cx", "cy"):
            self.register_buffer(name, torch.as_tensor(getattr(cameras, name)).float().reshape(-1).clone(), persistent=False)
        self.register_buffer("camera_type", ctype, persistent=False)
        self.register_buffer("distortion", dist, persistent=False)

    def forward(self, ray_indices: Tensor) -> RayBundle:
        """ray_indices `[num_rays,3]` = (camera, row, col) -> RayBundle (pixel centres at +0.5)."""
        if self.pinhole:
            o, d, pa, dn = F.raygen_pinhole(ray_indices, self.c2w, self.fx, self.fy, self.cx, self.cy)
        else:  # (the types were checked at construction)
            o, d, pa, dn = F.raygen_lens(ray_indices, self.c2w, self.fx, self.fy, self.cx, self.cy, self.camera_type,
                                         self.distortion, check_types=False)
        return RayBundle(
            origins=o,
            directions=d,
            pixel_area=pa,
            camera_indices=ray_indices[:, 0:1].to(torch.int64),
            metadata={"directions_norm": dn},
        )
