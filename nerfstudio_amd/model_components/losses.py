"""Losses on the nerfacto path (reference: nerfstudio/model_components/losses.py — MSELoss :31, interlevel_loss
:113-131, distortion_loss :149-154, orientation_loss :201-214, pred_normal_loss :217-222). The proposal losses are per-ray
fused value+gradient kernels (csrc/losses.hip); the two normals terms (predict_normals, off by default) are a handful of
elementwise torch ops on tensors the field already produced. Depth supervision (depth_loss :289-325 over ds_nerf_depth_loss
:225-247 and urban_radiance_field_depth_loss :250-286) is one more per-ray fused value+gradient kernel; depth_ranking_loss
:572-586 is the handful of torch ops it is."""
from enum import Enum
from typing import List, Optional

import torch
from torch import Tensor, nn

from .. import functional as F
from ..cameras.rays import RaySamples, pack_of, t_bins_of

MSELoss = nn.MSELoss
EPS = 1.0e-7


class DepthLossType(Enum):
    """Types of depth losses for depth supervision (losses.py:41-46)."""

    DS_NERF = 1
    URF = 2
    SPARSENERF_RANKING = 3


FORCE_PSEUDODEPTH_LOSS = False
PSEUDODEPTH_COMPATIBLE_LOSSES = (DepthLossType.SPARSENERF_RANKING,)


def ray_samples_to_sdist(ray_samples: RaySamples) -> Tensor:
    """Spacing-domain bin edges `[num_rays, S+1]` (losses.py:105-110)."""
    pk = pack_of(ray_samples)
    if pk is not None and pk.s_bins is not None:
        return pk.s_bins
    starts, ends = ray_samples.spacing_starts, ray_samples.spacing_ends
    return torch.cat([starts[..., 0], ends[..., -1:, 0]], dim=-1)


def interlevel_loss(weights_list: List[Tensor], ray_samples_list: List[RaySamples]) -> Tensor:
    """Proposal loss of mip-NeRF 360 (losses.py:113-131). weights `[N,S_i,1]`."""
    bins = [ray_samples_to_sdist(rs) for rs in ray_samples_list]
    ws = [w[..., 0] for w in weights_list]
    return F.interlevel_loss(ws, bins)


def distortion_loss(weights_list: List[Tensor], ray_samples_list: List[RaySamples]) -> Tensor:
    """Distortion loss of mip-NeRF 360 on the final level (losses.py:149-154)."""
    return F.distortion_loss(weights_list[-1][..., 0], ray_samples_to_sdist(ray_samples_list[-1]))


def orientation_loss(weights: Tensor, normals: Tensor, viewdirs: Tensor) -> Tensor:
    """Ref-NeRF orientation loss (losses.py:201-214): a visible normal should not point away from the camera. weights
    `[*bs,S,1]`, normals `[*bs,S,3]`, viewdirs `[*bs,3]` -> `[*bs]`: sum_s w_s min(0, n_s . (-d))^2."""
    towards_camera = -(normals * viewdirs[..., None, :]).sum(dim=-1)  # n . (-d); negation is exact
    back_facing = torch.fmin(towards_camera, torch.zeros_like(towards_camera))  # (fmin: a NaN dot product counts as 0)
    return (weights[..., 0] * back_facing**2).sum(dim=-1)


def pred_normal_loss(weights: Tensor, normals: Tensor, pred_normals: Tensor) -> Tensor:
    """Predicted normals against the ones computed from the density (losses.py:217-222): sum_s w_s (1 - n_s . p_s) -> `[*bs]`."""
    agreement = (normals * pred_normals).sum(dim=-1)
    return (weights[..., 0] * (1.0 - agreement)).sum(dim=-1)


def depth_loss_levels(weights_list: List[Tensor], ray_samples_list: List[RaySamples], termination_depth: Tensor,
                      predicted_depth: Optional[Tensor], sigma, directions_norm: Optional[Tensor], is_euclidean: bool,
                      depth_loss_type) -> Tensor:
    """The loop of DepthNerfactoModel.get_metrics_dict (models/depth_nerfacto.py:94-104) as ONE launch: the depth loss of every
    sampling level, averaged over the levels. weights `[N,S_i,1]`."""
    bins = [t_bins_of(rs) for rs in ray_samples_list]
    ws = [w[..., 0] for w in weights_list]
    return F.depth_loss(ws, bins, termination_depth, predicted_depth, sigma, directions_norm, is_euclidean,
                        int(getattr(depth_loss_type, "value", depth_loss_type)))


def depth_loss(weights: Tensor, ray_samples: RaySamples, termination_depth: Tensor, predicted_depth: Tensor, sigma,
               directions_norm: Tensor, is_euclidean: bool, depth_loss_type) -> Tensor:
    """Depth loss of one sampling level, the reference's signature (losses.py:289-325): weights `[N,S,1]`, termination_depth /
    predicted_depth / directions_norm `[N,1]`, sigma a one-element tensor or a float. DS_NERF and URF; anything else raises
    NotImplementedError as the reference does."""
    return depth_loss_levels([weights], [ray_samples], termination_depth, predicted_depth, sigma, directions_norm,
                             is_euclidean, depth_loss_type)


def depth_ranking_loss(rendered_depth: Tensor, gt_depth: Tensor) -> Tensor:
    """Depth ranking loss of SparseNeRF (losses.py:572-586); the batch comes from a PairPixelSampler, so neighbouring rows
    are pixels within a radius of each other."""
    m = 1e-4
    if rendered_depth.shape[0] % 2 != 0:  # chop off one index
        rendered_depth = rendered_depth[:-1, :]
        gt_depth = gt_depth[:-1, :]
    dpt_diff = gt_depth[::2, :] - gt_depth[1::2, :]
    out_diff = rendered_depth[::2, :] - rendered_depth[1::2, :] + m
    differing_signs = torch.sign(dpt_diff) != torch.sign(out_diff)
    return torch.nanmean(out_diff[differing_signs] * torch.sign(out_diff[differing_signs]))
