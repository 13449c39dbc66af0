"""depth-nerfacto over the HIP components: nerfacto plus a depth loss over the weights of every sampling level (reference:
nerfstudio/models/depth_nerfacto.py — config :34-53, populate_modules :65-72, get_outputs :74-78, get_metrics_dict :80-112,
get_loss_dict :114-126, get_image_metrics_and_images :128-149, _get_sigma :151-158).

DS_NERF and URF run as one launch of nsamd_depth_loss for all levels (functional.depth_loss); the ranking loss is a handful of
torch ops. The explicit schedule behind `fused_train_step` covers DS_NERF (train_step.NerfactoTrainStep.set_depth_target);
the captured trainer declines a depth model (pipeline.unsupported_model_reason).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import Tensor

from .cameras.rays import RayBundle
from .model_components import losses
from .model_components.losses import DepthLossType, depth_loss_levels, depth_ranking_loss
from .nerfacto import NerfactoModel, NerfactoModelConfig


@dataclass
class DepthNerfactoModelConfig(NerfactoModelConfig):
    """Additional parameters for depth supervision (models/depth_nerfacto.py:34-53)."""

    depth_loss_mult: float = 1e-3
    """Lambda of the depth loss."""
    is_euclidean_depth: bool = False
    """Whether input depth maps are Euclidean distances (or z-distances)."""
    depth_sigma: float = 0.01
    """Uncertainty around depth values in meters (defaults to 1cm)."""
    should_decay_sigma: bool = False
    """Whether to exponentially decay sigma."""
    starting_depth_sigma: float = 0.2
    """Starting uncertainty around depth values in meters (defaults to 0.2m)."""
    sigma_decay_rate: float = 0.99985
    """Rate of exponential decay."""
    depth_loss_type: DepthLossType = DepthLossType.DS_NERF
    """Depth loss type. SPARSENERF_RANKING expects the batch layout of a PairPixelSampler."""


def get_sigma(model) -> Tensor:
    """models/depth_nerfacto.py:151-158: the (one-element, host) sigma of this iteration, decayed when the config says so."""
    cfg = model.config
    if not cfg.should_decay_sigma:
        return model.depth_sigma
    model.depth_sigma = torch.maximum(cfg.sigma_decay_rate * model.depth_sigma, torch.tensor([cfg.depth_sigma]))
    return model.depth_sigma


def depth_metrics(model, outputs, batch, metrics_dict: dict) -> dict:
    """The training branch of DepthNerfactoModel.get_metrics_dict (models/depth_nerfacto.py:82-110) with the loop over the
    levels as one kernel launch. Shared by DepthNerfactoModel and the plugin's subclass of the reference's model."""
    cfg = model.config
    kind = cfg.depth_loss_type
    if losses.FORCE_PSEUDODEPTH_LOSS and kind not in losses.PSEUDODEPTH_COMPATIBLE_LOSSES:
        raise ValueError(f"Forcing pseudodepth loss, but depth loss type ({kind}) must be one of "
                         f"{losses.PSEUDODEPTH_COMPATIBLE_LOSSES}")
    value = int(getattr(kind, "value", kind))
    device = outputs["expected_depth"].device
    if value in (DepthLossType.DS_NERF.value, DepthLossType.URF.value):
        sigma = model._get_sigma()  # the model's own (the reference's, under the plugin): decays once per call
        metrics_dict["depth_loss"] = depth_loss_levels(
            outputs["weights_list"], outputs["ray_samples_list"], batch["depth_image"].to(device), outputs["expected_depth"],
            sigma, outputs.get("directions_norm"), cfg.is_euclidean_depth, value)
    elif value == DepthLossType.SPARSENERF_RANKING.value:
        metrics_dict["depth_ranking"] = depth_ranking_loss(outputs["expected_depth"], batch["depth_image"].to(device))
    else:
        raise NotImplementedError(f"Unknown depth loss type {kind}")
    return metrics_dict


def depth_loss_terms(model, loss_dict: dict, metrics_dict: Optional[dict]) -> dict:
    """models/depth_nerfacto.py:116-125."""
    assert metrics_dict is not None and ("depth_loss" in metrics_dict or "depth_ranking" in metrics_dict)
    cfg = model.config
    if "depth_ranking" in metrics_dict:
        loss_dict["depth_ranking"] = (cfg.depth_loss_mult * np.interp(model.step, [0, 2000], [0, 0.2])
                                      * metrics_dict["depth_ranking"])
    if "depth_loss" in metrics_dict:
        loss_dict["depth_loss"] = cfg.depth_loss_mult * metrics_dict["depth_loss"]
    return loss_dict


class DepthNerfactoModel(NerfactoModel):
    """Depth loss augmented nerfacto model."""

    config: DepthNerfactoModelConfig

    def populate_modules(self) -> None:
        super().populate_modules()
        c = self.config
        self.depth_sigma = torch.tensor([c.starting_depth_sigma if c.should_decay_sigma else c.depth_sigma])

    def _get_sigma(self) -> Tensor:
        return get_sigma(self)

    def get_outputs(self, ray_bundle: RayBundle, jitters: Optional[List[Tensor]] = None) -> Dict[str, object]:
        outputs = super().get_outputs(ray_bundle, jitters)
        if ray_bundle.metadata is not None and "directions_norm" in ray_bundle.metadata:
            outputs["directions_norm"] = ray_bundle.metadata["directions_norm"]
        return outputs

    def get_metrics_dict(self, outputs, batch) -> Dict[str, Tensor]:
        metrics_dict = super().get_metrics_dict(outputs, batch)
        if self.training and "fused_step" not in outputs:
            depth_metrics(self, outputs, batch, metrics_dict)
        return metrics_dict

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, Tensor]:
        loss_dict = super().get_loss_dict(outputs, batch, metrics_dict)
        if self.training and "fused_step" not in outputs:
            depth_loss_terms(self, loss_dict, metrics_dict)
        return loss_dict

    def get_image_metrics_and_images(self, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]):
        """What DepthNerfactoModel adds to the image metrics (models/depth_nerfacto.py:133-148): `depth_mse`, the MSE of the
        rendered depth over the pixels that have a ground-truth depth. This package's NerfactoModel leaves the rgb metrics and
        the colour-mapped images to the trainer, so the image dictionary is empty."""
        gt = batch["depth_image"].to(outputs["depth"].device)
        if not self.config.is_euclidean_depth:
            gt = gt * outputs["directions_norm"]
        mask = gt > 0
        return {"depth_mse": float(torch.nn.functional.mse_loss(outputs["depth"][mask], gt[mask]).cpu())}, {}
