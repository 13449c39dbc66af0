"""nerfacto wiring over the HIP components (reference: nerfstudio/models/nerfacto.py — config :46-133,
populate_modules :144-253, get_param_groups :255-260, callbacks :262-296, get_outputs :298-348, get_metrics_dict
:350-361, get_loss_dict :363-392; defaults overridden by configs/method_configs.py:87-121).

This is the caller of the hot path, kept thin: it instantiates the fields / sampler / renderers of this package with
the reference's hyper-parameters and reproduces the reference's control flow (proposal update schedule, weight
anneal, eval-mode switches). The trainer, datamanager, viewer and camera optimiser stay nerfstudio's.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Literal, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn
from torch.nn import Parameter

from . import eval_frame, eval_render
from .cameras.rays import RayBundle, RaySamples
from .field_components.field_heads import FieldHeadNames
from .field_components.spatial_distortions import SceneContraction
from .fields.density_fields import HashMLPDensityField
from .fields.nerfacto_field import NerfactoField
from .model_components.losses import MSELoss, distortion_loss, interlevel_loss, orientation_loss, pred_normal_loss
from .cameras.camera_optimizers import CameraOptimizer, CameraOptimizerConfig
from .model_components.ray_samplers import ProposalNetworkSampler
from .model_components.renderers import AccumulationRenderer, DepthRenderer, NormalsRenderer, RGBRenderer
from .model_components.shaders import NormalsShader
from .model_components.scene_colliders import NearFarCollider


@dataclass
class NerfactoModelConfig:
    """models/nerfacto.py:46-133 with the `nerfacto` method overrides (method_configs.py:99-103)."""

    near_plane: float = 0.05
    far_plane: float = 1000.0
    background_color: Literal["random", "last_sample", "black", "white"] = "last_sample"
    hidden_dim: int = 64
    hidden_dim_color: int = 64
    num_levels: int = 16
    base_res: int = 16
    max_res: int = 2048
    log2_hashmap_size: int = 19
    features_per_level: int = 2
    num_proposal_samples_per_ray: Tuple[int, ...] = (256, 96)
    num_nerf_samples_per_ray: int = 48
    proposal_initial_sampler: Literal["piecewise", "uniform"] = "piecewise"
    proposal_update_every: int = 5
    proposal_warmup: int = 5000
    num_proposal_iterations: int = 2
    use_same_proposal_network: bool = False
    proposal_net_args_list: List[Dict] = field(
        default_factory=lambda: [
            {"hidden_dim": 16, "log2_hashmap_size": 17, "num_levels": 5, "max_res": 128, "use_linear": False},
            {"hidden_dim": 16, "log2_hashmap_size": 17, "num_levels": 5, "max_res": 256, "use_linear": False},
        ]
    )
    interlevel_loss_mult: float = 1.0
    distortion_loss_mult: float = 0.002
    orientation_loss_mult: float = 0.0001
    pred_normal_loss_mult: float = 0.001
    predict_normals: bool = False
    """Analytic normals from the density gradient + the predicted-normals head (models/nerfacto.py:103-120, :325-345,
    :379-388). On the module path the field then runs as the reference composes it (fields/nerfacto_field.py here), not as the
    fused pipeline; with `fused_train_step` training runs the explicit schedule's normals stage (train_step.NerfactoTrainStep)."""
    use_proposal_weight_anneal: bool = True
    use_appearance_embedding: bool = True
    use_average_appearance_embedding: bool = True
    proposal_weights_anneal_slope: float = 10.0
    proposal_weights_anneal_max_num_iters: int = 1000
    use_single_jitter: bool = True
    use_gradient_scaling: bool = False
    """Scale the field gradients by the squared ray distance (models/nerfacto.py:114-115, :321-322)."""
    disable_scene_contraction: bool = False
    implementation: Literal["hip"] = "hip"
    appearance_embed_dim: int = 32
    average_init_density: float = 0.01
    eval_num_rays_per_chunk: int = 32768
    # models/nerfacto.py:131: the reference's default is CameraOptimizerConfig(mode="SO3xR3") (and the `nerfacto` method
    # config repeats it, method_configs.py:102); the Blender benchmark recipe turns it off
    # (scripts/benchmarking/launch_train_blender.sh:31) and so does this package's benchmark — the default here is "off",
    # `CameraOptimizerConfig(mode="SO3xR3")` enables the reference behaviour.
    camera_optimizer: CameraOptimizerConfig = field(default_factory=lambda: CameraOptimizerConfig(mode="off"))
    # Training iterations through the explicit kernel schedule behind this same Model API (fused_step.FusedTrainStep):
    # one autograd node instead of ~60, gradients written straight into param.grad — 2.3x faster than the module path
    # when a trainer drives the model eagerly. Not a reference field.
    fused_train_step: bool = False


class NerfactoModel(nn.Module):
    """The nerfacto graph on the MI355X kernels. `forward(ray_bundle)` = collider -> get_outputs
    (models/base_model.py:132-143)."""

    lpips = None  # a callable (gt [1,C,H,W], pred) -> scalar adds "lpips" to the image metrics; its weights are not part of this package

    def __init__(self, config: NerfactoModelConfig, aabb: Tensor, num_train_data: int) -> None:
        super().__init__()
        self.config = config
        self.register_buffer("aabb", aabb.float())
        self.num_train_data = num_train_data
        self.populate_modules()

    def populate_modules(self) -> None:
        c = self.config
        scene_contraction = None if c.disable_scene_contraction else SceneContraction(order=float("inf"))
        self.field = NerfactoField(
            self.aabb,
            hidden_dim=c.hidden_dim,
            num_levels=c.num_levels,
            max_res=c.max_res,
            base_res=c.base_res,
            features_per_level=c.features_per_level,
            log2_hashmap_size=c.log2_hashmap_size,
            hidden_dim_color=c.hidden_dim_color,
            spatial_distortion=scene_contraction,
            num_images=self.num_train_data,
            use_average_appearance_embedding=c.use_average_appearance_embedding,
            appearance_embedding_dim=c.appearance_embed_dim if c.use_appearance_embedding else 0,
            average_init_density=c.average_init_density,
            use_pred_normals=c.predict_normals,
            implementation=c.implementation,
        )
        # pose corrections of the training cameras (models/nerfacto.py:178-180; the parameter lives on the model's device)
        self.camera_optimizer: CameraOptimizer = c.camera_optimizer.setup(num_cameras=self.num_train_data, device="cpu")
        self.density_fns = []
        self.proposal_networks = nn.ModuleList()
        n_props = c.num_proposal_iterations
        n_nets = 1 if c.use_same_proposal_network else n_props
        for i in range(n_nets):
            args = c.proposal_net_args_list[min(i, len(c.proposal_net_args_list) - 1)]
            self.proposal_networks.append(
                HashMLPDensityField(self.aabb, spatial_distortion=scene_contraction, **args,
                                    average_init_density=c.average_init_density, implementation=c.implementation))
        if c.use_same_proposal_network:
            self.density_fns.extend([self.proposal_networks[0].density_fn for _ in range(n_props)])
        else:
            self.density_fns.extend([net.density_fn for net in self.proposal_networks])

        def update_schedule(step):  # models/nerfacto.py:208-213
            return np.clip(np.interp(step, [0, c.proposal_warmup], [0, c.proposal_update_every]), 1,
                           c.proposal_update_every)

        initial_sampler = None  # piecewise by default (models/nerfacto.py:215-218)
        if c.proposal_initial_sampler == "uniform":
            from .model_components.ray_samplers import UniformSampler

            initial_sampler = UniformSampler(single_jitter=c.use_single_jitter)
        self.proposal_sampler = ProposalNetworkSampler(
            initial_sampler=initial_sampler,
            num_nerf_samples_per_ray=c.num_nerf_samples_per_ray,
            num_proposal_samples_per_ray=c.num_proposal_samples_per_ray,
            num_proposal_network_iterations=c.num_proposal_iterations,
            single_jitter=c.use_single_jitter,
            update_sched=update_schedule,
        )
        self.collider = NearFarCollider(near_plane=c.near_plane, far_plane=c.far_plane)
        self.renderer_rgb = RGBRenderer(background_color=c.background_color)
        self.renderer_accumulation = AccumulationRenderer()
        self.renderer_depth = DepthRenderer(method="median")
        self.renderer_expected_depth = DepthRenderer(method="expected")
        self.renderer_normals = NormalsRenderer()
        self.normals_shader = NormalsShader()
        self.rgb_loss = MSELoss()
        self.step = 0
        self._fused = None  # fused_step.FusedTrainStep, built on first use (config.fused_train_step)

    # --- reference API -------------------------------------------------------------------------------------------
    def get_param_groups(self) -> Dict[str, List[Parameter]]:
        groups = {"proposal_networks": list(self.proposal_networks.parameters()), "fields": list(self.field.parameters())}
        self.camera_optimizer.get_param_groups(param_groups=groups)  # + "camera_opt" when the mode is not "off"
        return groups

    def get_param_groups_ordered(self) -> Dict[str, List[Parameter]]:
        """Same groups, main field first: the order arena.ParamArena lays them out in (the main-field gradients are
        complete first in the backward, so their all-reduce can overlap the proposal-network backward)."""
        g = self.get_param_groups()
        out = {"fields": g["fields"], "proposal_networks": g["proposal_networks"]}
        if "camera_opt" in g:
            out["camera_opt"] = g["camera_opt"]
        return out

    def set_step(self, step: int) -> None:
        """BEFORE_TRAIN_ITERATION callback: proposal weight anneal (models/nerfacto.py:270-280)."""
        self.step = step
        if self.config.use_proposal_weight_anneal:
            n = self.config.proposal_weights_anneal_max_num_iters
            frac = np.clip(step / n, 0, 1)
            b = self.config.proposal_weights_anneal_slope
            self.proposal_sampler.set_anneal(float(b * frac / ((b - 1) * frac + 1)))

    def after_step(self, step: int) -> None:
        """AFTER_TRAIN_ITERATION callback (ray_samplers.py:571-574)."""
        self.proposal_sampler.step_cb(step)

    def forward(self, ray_bundle: RayBundle, jitters: Optional[List[Tensor]] = None) -> Dict[str, object]:
        ray_bundle = self.collider(ray_bundle)
        return self.get_outputs(ray_bundle, jitters)

    def _fused_step(self):
        """The FusedTrainStep of this model when config.fused_train_step asks for it and the configuration allows it."""
        if not (self.training and getattr(self.config, "fused_train_step", False) and torch.is_grad_enabled()):
            return None
        if self._fused is None:
            from .fused_step import FusedTrainStep

            self._fused = FusedTrainStep(self)
            reason = self._fused.supported()
            if reason is not None:
                raise NotImplementedError(f"fused_train_step: {reason} is only on the module path")
        return self._fused

    def get_outputs(self, ray_bundle: RayBundle, jitters: Optional[List[Tensor]] = None) -> Dict[str, object]:
        fused = self._fused_step()
        if fused is not None:
            return fused.get_outputs(ray_bundle, jitters)
        if self.training:  # apply the camera optimizer pose tweaks (models/nerfacto.py:299-301)
            self.camera_optimizer.apply_to_raybundle(ray_bundle)
        ray_samples: RaySamples
        ray_samples, weights_list, ray_samples_list = self.proposal_sampler(ray_bundle, density_fns=self.density_fns,
                                                                            jitters=jitters)
        field_outputs = self.field.forward(ray_samples, compute_normals=self.config.predict_normals)
        if self.config.use_gradient_scaling:  # models/nerfacto.py:321-322
            from . import functional as F

            dens, rgb_s = F.scale_gradients_by_distance_squared(field_outputs[FieldHeadNames.DENSITY], field_outputs[FieldHeadNames.RGB],
                                                                ray_samples.pack.t_bins)
            field_outputs = dict(field_outputs)
            field_outputs[FieldHeadNames.DENSITY], field_outputs[FieldHeadNames.RGB] = dens, rgb_s
        weights = ray_samples.get_weights(field_outputs[FieldHeadNames.DENSITY])
        weights_list.append(weights)
        ray_samples_list.append(ray_samples)
        if self.training:
            # RGBRenderer + AccumulationRenderer + DepthRenderer("expected") share one pass over the samples:
            # a single composite launch (csrc/render.hip) instead of the reference's three module calls.
            from . import functional as F

            rgb, acc1, dep1 = F.composite(field_outputs[FieldHeadNames.RGB], weights[..., 0], ray_samples.pack.t_bins,
                                          self.renderer_rgb.background_color, expected_depth=True)
            accumulation, expected_depth = acc1[:, None], dep1[:, None]
        else:
            rgb = self.renderer_rgb(rgb=field_outputs[FieldHeadNames.RGB], weights=weights)
            expected_depth = self.renderer_expected_depth(weights=weights, ray_samples=ray_samples)
            accumulation = self.renderer_accumulation(weights=weights)
        with torch.no_grad():
            depth = self.renderer_depth(weights=weights, ray_samples=ray_samples)
        outputs: Dict[str, object] = {"rgb": rgb, "accumulation": accumulation, "depth": depth,
                                      "expected_depth": expected_depth}
        if self.config.predict_normals:  # models/nerfacto.py:325-329
            normals = self.renderer_normals(normals=field_outputs[FieldHeadNames.NORMALS], weights=weights)
            pred_normals = self.renderer_normals(field_outputs[FieldHeadNames.PRED_NORMALS], weights=weights)
            outputs["normals"] = self.normals_shader(normals)
            outputs["pred_normals"] = self.normals_shader(pred_normals)
        if self.training:
            outputs["weights_list"] = weights_list
            outputs["ray_samples_list"] = ray_samples_list
        if self.training and self.config.predict_normals:  # models/nerfacto.py:335-344
            outputs["rendered_orientation_loss"] = orientation_loss(
                weights.detach(), field_outputs[FieldHeadNames.NORMALS], ray_bundle.directions)
            outputs["rendered_pred_normal_loss"] = pred_normal_loss(
                weights.detach(), field_outputs[FieldHeadNames.NORMALS].detach(), field_outputs[FieldHeadNames.PRED_NORMALS])
        for i in range(self.config.num_proposal_iterations):
            outputs[f"prop_depth_{i}"] = self.renderer_depth(weights=weights_list[i], ray_samples=ray_samples_list[i])
        return outputs

    def get_metrics_dict(self, outputs, batch) -> Dict[str, Tensor]:
        if "fused_step" in outputs:
            return outputs["fused_step"].get_metrics_dict(outputs, batch)
        metrics = {}
        gt = self.renderer_rgb.blend_background(batch["image"].to(outputs["rgb"].device))
        mse = torch.mean((outputs["rgb"].detach() - gt) ** 2)
        metrics["psnr"] = -10.0 * torch.log10(mse)
        if self.training:
            metrics["distortion"] = distortion_loss(outputs["weights_list"], outputs["ray_samples_list"])
        self.camera_optimizer.get_metrics_dict(metrics)
        return metrics

    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, Tensor]:
        if "fused_step" in outputs:
            return outputs["fused_step"].get_loss_dict(outputs, batch)
        image = batch["image"].to(outputs["rgb"].device)
        pred_rgb, gt_rgb = self.renderer_rgb.blend_background_for_loss_computation(
            pred_image=outputs["rgb"], pred_accumulation=outputs["accumulation"], gt_image=image)
        loss_dict = {"rgb_loss": self.rgb_loss(gt_rgb, pred_rgb)}
        if self.training:
            loss_dict["interlevel_loss"] = self.config.interlevel_loss_mult * interlevel_loss(
                outputs["weights_list"], outputs["ray_samples_list"])
            assert metrics_dict is not None and "distortion" in metrics_dict
            loss_dict["distortion_loss"] = self.config.distortion_loss_mult * metrics_dict["distortion"]
            if self.config.predict_normals:  # models/nerfacto.py:379-388
                loss_dict["orientation_loss"] = self.config.orientation_loss_mult * torch.mean(
                    outputs["rendered_orientation_loss"])
                loss_dict["pred_normal_loss"] = self.config.pred_normal_loss_mult * torch.mean(
                    outputs["rendered_pred_normal_loss"])
            self.camera_optimizer.get_loss_dict(loss_dict)  # L2 regulariser on the pose corrections
        return loss_dict

    def get_image_metrics_and_images(self, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]):
        """models/nerfacto.py:393-431: PSNR and SSIM of the frame on the device, read once as Python floats, and the
        reference's images_dict (eval.image_metrics_and_images). "lpips" only with a callable `self.lpips`."""
        from . import eval as eval_images

        return eval_images.image_metrics_and_images(self, outputs, batch)

    @torch.no_grad()
    def get_outputs_for_camera(self, camera, obb_box=None) -> Dict[str, Tensor]:
        """models/base_model.py:166-175. Eval mode, one perspective camera (undistorted, or with OpenCV distortion parameters),
        no crop box: the rays of each chunk are generated inside the device-side chunk loop
        (eval_render.EvalRenderer.render_camera) — no [H, W] bundle in HBM; anything else generates the bundle
        (`camera.generate_rays(camera_indices=0, keep_shape=True)`) and takes the loop below. Fisheye and equirectangular
        cameras are among "anything else" here; `render_camera(lens=...)` and RayGenerator generate their rays."""
        return eval_frame.outputs_for_camera(self, camera, obb_box, eval_render.runner_for)

    @torch.no_grad()
    def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle: RayBundle) -> Dict[str, Tensor]:
        """Chunked full-image render (models/base_model.py:178-205). In eval mode on the GPU the chunk loop is device-side
        (eval_render.EvalRenderer: one captured kernel schedule per chunk over static buffers, outputs copied into
        preallocated image buffers — no per-chunk module graph, no torch.cat); NSAMD_EVAL_RUNNER=0, training mode or an
        unsupported configuration take the reference's Python loop over `forward`."""
        return eval_frame.outputs_for_bundle(self, camera_ray_bundle, eval_render.runner_for)
