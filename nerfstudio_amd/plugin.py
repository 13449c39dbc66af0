"""`nerfacto-hip`: this package as an external nerfstudio method (no edits to nerfstudio).

nerfstudio discovers methods from the `nerfstudio.method_configs` entry-point group or from
`NERFSTUDIO_METHOD_CONFIGS="nerfacto-hip=nerfstudio_amd.plugin:nerfacto_hip"` (plugins/registry.py:34-78); an entry is a
`MethodSpecification(config: TrainerConfig, description)` (plugins/types.py:28-38). `nerfacto_hip()` builds it: the
reference's own `method_configs["nerfacto"]` (configs/method_configs.py:87-121) with the model config's `_target` pointing
at `HipNerfactoModel` — the reference's NerfactoModel whose hot-path modules (`field`, `proposal_networks`,
`proposal_sampler`, the renderers and the proposal losses) are replaced by the gfx950 implementations of this package
after `populate_modules()` (models/nerfacto.py:144-253). Everything else of nerfstudio (trainer, datamanager, viewer,
camera optimizer, metrics) is used as is; parameter names and shapes are unchanged, so checkpoints interchange.

nerfstudio itself is imported lazily: this module imports (and `install_hip_modules` works on any object with the
reference model's attributes) without nerfstudio installed; `nerfacto_hip()` raises ImportError with the reason then.
"""
from __future__ import annotations

from typing import Any, Optional, Callable, List

import numpy as np
import torch

DESCRIPTION = ("nerfacto on MI355X: hash encoding, fused density / colour MLPs, proposal sampling, compositing and the "
               "proposal losses as hand-written gfx950 HIP kernels (nerfstudio_amd, implementation='hip')")


def install_hip_modules(model: Any) -> None:
    """Swap the hot-path modules of a populated (reference) NerfactoModel for this package's. Uses only what
    `NerfactoModel.populate_modules` itself uses: `model.config` (NerfactoModelConfig fields), `model.scene_box.aabb`,
    `model.num_train_data`. Mirrors models/nerfacto.py:147-240 line by line, with the hip classes."""
    from .field_components.spatial_distortions import SceneContraction
    from .fields.density_fields import HashMLPDensityField
    from .fields.nerfacto_field import NerfactoField
    from .model_components.ray_samplers import ProposalNetworkSampler, UniformSampler
    from .model_components.renderers import AccumulationRenderer, DepthRenderer, RGBRenderer

    cfg = model.config
    if getattr(cfg, "features_per_level", 2) != 2:
        raise ValueError("nerfacto-hip: features_per_level must be 2")
    aabb = model.scene_box.aabb
    contraction = None if cfg.disable_scene_contraction else SceneContraction(order=float("inf"))
    app_dim = cfg.appearance_embed_dim if cfg.use_appearance_embedding else 0
    model.field = NerfactoField(
        aabb, hidden_dim=cfg.hidden_dim, num_levels=cfg.num_levels, max_res=cfg.max_res, base_res=cfg.base_res,
        features_per_level=cfg.features_per_level, log2_hashmap_size=cfg.log2_hashmap_size,
        hidden_dim_color=cfg.hidden_dim_color, spatial_distortion=contraction, num_images=model.num_train_data,
        use_average_appearance_embedding=cfg.use_average_appearance_embedding, appearance_embedding_dim=app_dim,
        average_init_density=cfg.average_init_density, use_pred_normals=getattr(cfg, "predict_normals", False),
        implementation="hip")
    nets = torch.nn.ModuleList()
    density_fns: List[Callable] = []
    n_prop = cfg.num_proposal_iterations
    if cfg.use_same_proposal_network:
        assert len(cfg.proposal_net_args_list) == 1, "Only one proposal network is allowed."
        net = HashMLPDensityField(aabb, spatial_distortion=contraction, **cfg.proposal_net_args_list[0],
                                  average_init_density=cfg.average_init_density, implementation="hip")
        nets.append(net)
        density_fns.extend([net.density_fn for _ in range(n_prop)])
    else:
        for i in range(n_prop):
            args = cfg.proposal_net_args_list[min(i, len(cfg.proposal_net_args_list) - 1)]
            nets.append(HashMLPDensityField(aabb, spatial_distortion=contraction, **args,
                                            average_init_density=cfg.average_init_density, implementation="hip"))
        density_fns.extend([net.density_fn for net in nets])
    model.proposal_networks, model.density_fns = nets, density_fns

    def update_schedule(step):  # models/nerfacto.py:208-213
        return np.clip(np.interp(step, [0, cfg.proposal_warmup], [0, cfg.proposal_update_every]), 1,
                       cfg.proposal_update_every)

    initial = UniformSampler(single_jitter=cfg.use_single_jitter) if cfg.proposal_initial_sampler == "uniform" else None
    model.proposal_sampler = ProposalNetworkSampler(
        num_nerf_samples_per_ray=cfg.num_nerf_samples_per_ray,
        num_proposal_samples_per_ray=cfg.num_proposal_samples_per_ray,
        num_proposal_network_iterations=cfg.num_proposal_iterations, single_jitter=cfg.use_single_jitter,
        update_sched=update_schedule, initial_sampler=initial)
    model.renderer_rgb = RGBRenderer(background_color=cfg.background_color)
    model.renderer_accumulation = AccumulationRenderer()
    model.renderer_depth = DepthRenderer(method="median")
    model.renderer_expected_depth = DepthRenderer(method="expected")


def hip_loss_terms(model: Any, outputs: dict, loss_dict: dict, metrics_dict: Optional[dict] = None) -> dict:
    """The proposal losses of NerfactoModel.get_loss_dict (models/nerfacto.py:363-375) through the fused kernels; the
    distortion term is taken from `metrics_dict["distortion"]` when get_metrics_dict already evaluated it (as the
    reference does, :374-375)."""
    from .model_components.losses import distortion_loss, interlevel_loss

    cfg = model.config
    loss_dict["interlevel_loss"] = cfg.interlevel_loss_mult * interlevel_loss(outputs["weights_list"], outputs["ray_samples_list"])
    dist = metrics_dict["distortion"] if metrics_dict is not None and "distortion" in metrics_dict else \
        distortion_loss(outputs["weights_list"], outputs["ray_samples_list"])
    loss_dict["distortion_loss"] = cfg.distortion_loss_mult * dist
    return loss_dict


def _publish(*classes):
    """Classes that need nerfstudio to be built become module-level names (pickle of the TrainerConfig for `mp.spawn`,
    scripts/train.py:205; yaml of `config.yml`, utils/eval_utils.py:90 — both resolve `module.qualname`)."""
    for cls in classes:
        cls.__module__ = __name__
        cls.__qualname__ = cls.__name__
        globals()[cls.__name__] = cls
    return classes


def _flush_pending(model: Any) -> None:
    """A pending (deferred / pipelined) main-field update of the pipeline's captured schedule is applied before the
    parameters are read (pipeline.EngineSeam.attach_optimizers installs the `_hip_flush` hook)."""
    getattr(model, "_hip_flush", lambda: None)()


def _nerfacto_eval_runner(model: Any, device):
    """HipNerfactoModel's device-side eval loop for rays on `device`, or None: the reference's own loop. The loop samples between
    the config's near / far planes: only a model whose collider does too takes it, for rays on the model's device."""
    from . import eval_render

    col, cfg = getattr(model, "collider", None), model.config
    planes = (getattr(col, "near_plane", None), getattr(col, "far_plane", None)) == (cfg.near_plane, cfg.far_plane)
    return eval_render.runner_for(model, device) if planes and torch.device(device) == torch.device(model.device) else None


def nerfacto_outputs_for_camera(model: Any, camera, obb_box, reference_path):
    """HipNerfactoModel.get_outputs_for_camera. One perspective camera (undistorted, or with OpenCV distortion parameters) without
    a crop box, in eval mode on the model's GPU: the rays of every chunk are generated inside the device-side chunk loop
    (EvalRenderer.render_camera over nsamd_raygen_pinhole_grid / nsamd_raygen_lens_grid: the arithmetic of
    `camera.generate_rays(camera_indices=0, keep_shape=True)`, cameras/cameras.py:321-503) — no [H, W] ray bundle is built.
    Anything else — fisheye and equirectangular cameras included, which `render_camera(lens=...)` covers — is
    `reference_path`, the reference's own method."""
    from . import eval_frame

    _flush_pending(model)
    return eval_frame.outputs_for_camera(model, camera, obb_box, _nerfacto_eval_runner, reference_path)


def nerfacto_outputs_for_camera_ray_bundle(model: Any, camera_ray_bundle, reference_path):
    """HipNerfactoModel.get_outputs_for_camera_ray_bundle. In eval mode, with the rays already on the model's GPU, the chunk loop
    is the device-side one (eval_render.EvalRenderer: one captured kernel schedule per chunk over static buffers, no
    per-chunk module graph, no torch.cat — 30.5 against 23.3 M rays/s, profiles/r03_final2_bench_render_*.json; same
    outputs bit for bit, tests/test_gpu_kernels.py); anything else takes `reference_path`, the reference's own loop.
    NSAMD_EVAL_RUNNER=0 switches it off."""
    from . import eval_frame

    _flush_pending(model)
    return eval_frame.outputs_for_bundle(model, camera_ray_bundle, _nerfacto_eval_runner, reference_path)


def _model_classes():
    """(HipNerfactoModelConfig, HipNerfactoModel), built ONCE against the installed nerfstudio."""
    if "HipNerfactoModel" in globals():
        return globals()["HipNerfactoModelConfig"], globals()["HipNerfactoModel"]
    from dataclasses import dataclass, field
    from typing import Literal, Type

    from nerfstudio.models.nerfacto import NerfactoModel, NerfactoModelConfig

    class HipNerfactoModel(NerfactoModel):
        """The reference NerfactoModel with the hot path on MI355X kernels."""

        def populate_modules(self):
            super().populate_modules()
            install_hip_modules(self)
            self._fused = None

        # config.fused_train_step: training iterations through fused_step.FusedTrainStep (same Model API, the explicit
        # kernel schedule underneath, gradients written straight into param.grad); everything else as the reference
        def _fused_step(self):
            if not (self.training and getattr(self.config, "fused_train_step", False) and torch.is_grad_enabled()):
                return None
            if self._fused is None:
                from .fused_step import FusedTrainStep

                self._fused = FusedTrainStep(self)
                reason = self._fused.supported()
                if reason is not None:
                    raise NotImplementedError(f"fused_train_step: {reason} is only on the module path")
            return self._fused

        def get_outputs(self, ray_bundle):
            fused = self._fused_step()
            return fused.get_outputs(ray_bundle) if fused is not None else super().get_outputs(ray_bundle)

        def train(self, mode: bool = True):  # the viewer and the evaluation entry points switch the MODEL to eval
            if not mode:
                _flush_pending(self)
            return super().train(mode)

        @torch.no_grad()
        def get_outputs_for_camera(self, camera, obb_box=None):  # models/base_model.py:162-176 (viewer, ns-render)
            return nerfacto_outputs_for_camera(self, camera, obb_box, super().get_outputs_for_camera)

        @torch.no_grad()
        def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle):  # models/base_model.py:178-205
            return nerfacto_outputs_for_camera_ray_bundle(self, camera_ray_bundle, super().get_outputs_for_camera_ray_bundle)

        def get_loss_dict(self, outputs, batch, metrics_dict=None):
            """models/nerfacto.py:363-392 with the proposal losses on the fused HIP kernels (the reference's torch
            `interlevel_loss` builds [N,S,S] temporaries and ~20 eager launches per level)."""
            if "fused_step" in outputs:
                return outputs["fused_step"].get_loss_dict(outputs, batch)
            if not self.training:
                return super().get_loss_dict(outputs, batch, metrics_dict)
            loss_dict = {}
            image = batch["image"].to(self.device)
            pred_rgb, gt_rgb = self.renderer_rgb.blend_background_for_loss_computation(
                pred_image=outputs["rgb"], pred_accumulation=outputs["accumulation"], gt_image=image)
            loss_dict["rgb_loss"] = self.rgb_loss(gt_rgb, pred_rgb)
            hip_loss_terms(self, outputs, loss_dict, metrics_dict)
            if self.config.predict_normals:  # models/nerfacto.py:379-388 (the terms were rendered by get_outputs, :335-344)
                loss_dict["orientation_loss"] = self.config.orientation_loss_mult * torch.mean(
                    outputs["rendered_orientation_loss"])
                loss_dict["pred_normal_loss"] = self.config.pred_normal_loss_mult * torch.mean(
                    outputs["rendered_pred_normal_loss"])
            self.camera_optimizer.get_loss_dict(loss_dict)
            return loss_dict

        def get_metrics_dict(self, outputs, batch):
            from .model_components.losses import distortion_loss

            if "fused_step" in outputs:
                return outputs["fused_step"].get_metrics_dict(outputs, batch)
            metrics = {}
            gt_rgb = self.renderer_rgb.blend_background(batch["image"].to(self.device))
            metrics["psnr"] = self.psnr(outputs["rgb"], gt_rgb)
            if self.training:
                metrics["distortion"] = distortion_loss(outputs["weights_list"], outputs["ray_samples_list"])
            self.camera_optimizer.get_metrics_dict(metrics)
            return metrics

    @dataclass
    class HipNerfactoModelConfig(NerfactoModelConfig):
        _target: Type = field(default_factory=lambda: HipNerfactoModel)
        implementation: Literal["tcnn", "torch", "hip"] = "hip"
        fused_train_step: bool = False
        """Run training iterations on the explicit kernel schedule behind the Model API (nerfstudio_amd/fused_step.py)."""

    _publish(HipNerfactoModelConfig, HipNerfactoModel)
    return HipNerfactoModelConfig, HipNerfactoModel


# ---------------------------------------------------------------------------------------------------------------------
# instant-ngp (BASELINE configs[3]): the same construction for the reference's NGPModel
# ---------------------------------------------------------------------------------------------------------------------
NGP_DESCRIPTION = ("instant-ngp on MI355X: occupancy-grid marching, packed transmittance scan with early termination, hash "
                   "encoding + fused MLPs and packed compositing as hand-written gfx950 HIP kernels (nerfstudio_amd)")


def install_hip_ngp_modules(model: Any) -> None:
    """Swap the hot-path modules of a populated (reference) NGPModel for this package's; mirrors models/instant_ngp.py:96-137
    with the hip classes. What nerfacc provides there (OccGridEstimator) is model_components/occupancy.py here."""
    from .field_components.spatial_distortions import SceneContraction
    from .fields.nerfacto_field import NerfactoField
    from .model_components.occupancy import OccGridEstimator
    from .model_components.ray_samplers import VolumetricSampler
    from .model_components.renderers import AccumulationRenderer, DepthRenderer, RGBRenderer

    cfg = model.config
    if not isinstance(cfg.grid_resolution, int):
        raise ValueError("instant-ngp-hip: grid_resolution must be one integer (a cubic grid)")
    contraction = None if cfg.disable_scene_contraction else SceneContraction(order=float("inf"))
    model.field = NerfactoField(
        aabb=model.scene_box.aabb,
        # (sic) models/instant_ngp.py:104: the embedding is 32 wide when use_appearance_embedding is FALSE, as upstream
        appearance_embedding_dim=0 if cfg.use_appearance_embedding else 32,
        num_images=model.num_train_data, log2_hashmap_size=cfg.log2_hashmap_size, max_res=cfg.max_res,
        spatial_distortion=contraction)
    if cfg.render_step_size is None:  # (the reference's populate_modules has normally set it already, :113-115)
        a = model.scene_box.aabb.flatten()
        cfg.render_step_size = float(((a[3:] - a[:3]) ** 2).sum().sqrt().item() / 1000)
    model.occupancy_grid = OccGridEstimator(roi_aabb=model.scene_box.aabb.flatten(), resolution=cfg.grid_resolution,
                                            levels=cfg.grid_levels)
    model.sampler = VolumetricSampler(occupancy_grid=model.occupancy_grid, density_fn=model.field.density_fn)
    model.renderer_rgb = RGBRenderer(background_color=cfg.background_color)
    model.renderer_accumulation = AccumulationRenderer()
    model.renderer_depth = DepthRenderer(method="expected")


def _ngp_eval_runner(model: Any, device):
    """HipNGPModel's device-side eval loop for rays on `device`, or None: the reference's own loop. Model.forward puts a
    collider's nears / fars on every chunk (models/base_model.py:140-141); instant-ngp has none (models/instant_ngp.py:48-51),
    and only such a model takes the device-side loop, for rays on the model's device."""
    from . import ngp_eval_render

    own = getattr(model, "collider", None) is None and torch.device(device) == torch.device(model.device)
    return ngp_eval_render.runner_for(model, device) if own else None


def ngp_outputs_for_camera(model: Any, camera, obb_box, reference_path):
    """HipNGPModel.get_outputs_for_camera. One perspective camera without a crop box, in eval mode on the model's GPU: the rays
    of every chunk are generated inside the device-side chunk loop (ngp_eval_render.NgpEvalRenderer.render_camera). Anything
    else is `reference_path`, the reference's own method: its bundle — with a crop box's nears / fars — comes back through
    `ngp_outputs_for_camera_ray_bundle`. A pending parameter update is applied first, as for HipNerfactoModel."""
    from . import eval_frame

    _flush_pending(model)
    return eval_frame.outputs_for_camera(model, camera, obb_box, _ngp_eval_runner, reference_path)


def ngp_outputs_for_camera_ray_bundle(model: Any, camera_ray_bundle, reference_path):
    """HipNGPModel.get_outputs_for_camera_ray_bundle. In eval mode, with the rays already on the model's GPU, the chunk loop is
    the device-side one (ngp_eval_render.NgpEvalRenderer); anything else takes `reference_path`, the reference's own loop.
    NSAMD_EVAL_RUNNER=0 switches it off."""
    from . import eval_frame

    _flush_pending(model)
    return eval_frame.outputs_for_bundle(model, camera_ray_bundle, _ngp_eval_runner, reference_path)


def _ngp_model_classes():
    """(HipInstantNGPModelConfig, HipNGPModel), built ONCE against the installed nerfstudio (which imports nerfacc)."""
    if "HipNGPModel" in globals():
        return globals()["HipInstantNGPModelConfig"], globals()["HipNGPModel"]
    from dataclasses import dataclass, field
    from typing import Type

    from nerfstudio.models.instant_ngp import InstantNGPModelConfig, NGPModel

    class HipNGPModel(NGPModel):
        """The reference NGPModel with the hot path on MI355X kernels: its callbacks (occupancy refresh every step's
        BEFORE_TRAIN_ITERATION, models/instant_ngp.py:150-163), parameter groups, metrics and loss are the reference's own
        code over the swapped modules; get_outputs is this package's (the reference's calls nerfacc directly, :191-198)."""

        def populate_modules(self):
            super().populate_modules()
            install_hip_ngp_modules(self)
            self._fused = None

        def _fused_step(self):
            if not (self.training and getattr(self.config, "fused_train_step", False) and torch.is_grad_enabled()):
                return None
            if getattr(self.config, "use_gradient_scaling", False):
                raise NotImplementedError("fused_train_step: use_gradient_scaling is only on the module path")
            from .fused_step import ddp_reason

            if ddp_reason() is not None:
                raise NotImplementedError(f"fused_train_step: {ddp_reason()} is only on the module path")
            if self._fused is None:
                from .ngp_step import NgpFusedStep

                self._fused = NgpFusedStep(self)
            return self._fused

        def get_outputs(self, ray_bundle):
            from .instant_ngp import ngp_outputs

            fused = self._fused_step()
            return fused.get_outputs(ray_bundle) if fused is not None else ngp_outputs(self, ray_bundle)

        def get_loss_dict(self, outputs, batch, metrics_dict=None):
            if "ngp_step" in outputs:
                return outputs["ngp_step"].get_loss_dict(outputs, batch)
            return super().get_loss_dict(outputs, batch, metrics_dict)

        @torch.no_grad()
        def get_outputs_for_camera(self, camera, obb_box=None):  # models/base_model.py:165-175 (viewer, ns-render)
            return ngp_outputs_for_camera(self, camera, obb_box, super().get_outputs_for_camera)

        @torch.no_grad()
        def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle):  # models/base_model.py:177-205
            return ngp_outputs_for_camera_ray_bundle(self, camera_ray_bundle, super().get_outputs_for_camera_ray_bundle)

    @dataclass
    class HipInstantNGPModelConfig(InstantNGPModelConfig):
        _target: Type = field(default_factory=lambda: HipNGPModel)
        fused_train_step: bool = False
        """Run training iterations on the explicit kernel schedule behind the Model API (nerfstudio_amd/ngp_step.py)."""

    _publish(HipInstantNGPModelConfig, HipNGPModel)
    return HipInstantNGPModelConfig, HipNGPModel


# ---------------------------------------------------------------------------------------------------------------------
# depth-nerfacto: the reference's DepthNerfactoModel over the same hot-path modules, its depth loss on nsamd_depth_loss
# ---------------------------------------------------------------------------------------------------------------------
DEPTH_DESCRIPTION = ("depth-nerfacto on MI355X: nerfacto-hip plus the DS-NeRF / Urban Radiance Fields depth loss over the "
                     "weights of every sampling level as one gfx950 HIP kernel (nerfstudio_amd)")


def _depth_model_classes():
    """(HipDepthNerfactoModelConfig, HipDepthNerfactoModel), built ONCE against the installed nerfstudio."""
    if "HipDepthNerfactoModel" in globals():
        return globals()["HipDepthNerfactoModelConfig"], globals()["HipDepthNerfactoModel"]
    from dataclasses import dataclass, field
    from typing import Literal, Type

    from nerfstudio.models.depth_nerfacto import DepthNerfactoModel, DepthNerfactoModelConfig

    _, hip_nerfacto = _model_classes()

    class HipDepthNerfactoModel(hip_nerfacto, DepthNerfactoModel):
        """The reference DepthNerfactoModel with the hot path on MI355X kernels. HipNerfactoModel comes first in the method
        resolution order: its populate_modules / get_outputs call on into the reference's DepthNerfactoModel (`depth_sigma`,
        `directions_norm` in the outputs), `_get_sigma` and the image metrics are the reference's own code, and the loop of depth
        losses over the levels (models/depth_nerfacto.py:94-104) is one launch of nsamd_depth_loss."""

        def get_metrics_dict(self, outputs, batch):
            from .depth_nerfacto import depth_metrics

            metrics_dict = hip_nerfacto.get_metrics_dict(self, outputs, batch)
            if self.training and "fused_step" not in outputs:
                depth_metrics(self, outputs, batch, metrics_dict)
            return metrics_dict

        def get_loss_dict(self, outputs, batch, metrics_dict=None):
            from .depth_nerfacto import depth_loss_terms

            loss_dict = hip_nerfacto.get_loss_dict(self, outputs, batch, metrics_dict)
            if self.training and "fused_step" not in outputs:
                depth_loss_terms(self, loss_dict, metrics_dict)
            return loss_dict

    @dataclass
    class HipDepthNerfactoModelConfig(DepthNerfactoModelConfig):
        _target: Type = field(default_factory=lambda: HipDepthNerfactoModel)
        implementation: Literal["tcnn", "torch", "hip"] = "hip"
        fused_train_step: bool = False
        """Run training iterations on the explicit kernel schedule behind the Model API (DS_NERF only; fused_step.py)."""

    _publish(HipDepthNerfactoModelConfig, HipDepthNerfactoModel)
    return HipDepthNerfactoModelConfig, HipDepthNerfactoModel


def depth_nerfacto_hip():
    """-> MethodSpecification for `ns-train depth-nerfacto-hip` (the reference's `depth-nerfacto` recipe,
    method_configs.py:215-249: its depth datamanager, optimisers and pipeline). Reached through
    NERFSTUDIO_METHOD_CONFIGS="depth-nerfacto-hip=nerfstudio_amd.plugin:depth_nerfacto_hip"; the iterations run on the module
    path (pipeline.unsupported_model_reason: "depth supervision"). Raises ImportError when nerfstudio is not importable."""
    import copy
    import dataclasses

    try:
        from nerfstudio.configs.method_configs import method_configs
        from nerfstudio.plugins.types import MethodSpecification
    except Exception as e:  # noqa: BLE001
        raise ImportError(f"nerfstudio_amd.plugin: nerfstudio (with its trainer dependencies) is not importable: {e}") from e
    from .utils import profiler

    profiler.hook_reference_profiler()
    cfg_cls, _ = _depth_model_classes()
    base = copy.deepcopy(method_configs["depth-nerfacto"])
    old = base.pipeline.model
    kwargs = {f.name: getattr(old, f.name) for f in dataclasses.fields(old) if f.name not in ("_target", "implementation")}
    base.pipeline.model = cfg_cls(**kwargs)
    base.method_name = "depth-nerfacto-hip"
    base.mixed_precision = False  # fp32 kernels: no autocast, no loss scaling
    return MethodSpecification(config=base, description=DEPTH_DESCRIPTION)


def instant_ngp_hip():
    """-> MethodSpecification for `ns-train instant-ngp-hip` (the reference's `instant-ngp` recipe, method_configs.py:251-273:
    DynamicBatchPipeline, one Adam group). Raises ImportError when nerfstudio is not importable."""
    import copy
    import dataclasses

    try:
        from nerfstudio.configs.method_configs import method_configs
        from nerfstudio.plugins.types import MethodSpecification
    except Exception as e:  # noqa: BLE001
        raise ImportError(f"nerfstudio_amd.plugin: nerfstudio (with its trainer dependencies) is not importable: {e}") from e
    from .utils import profiler

    profiler.hook_reference_profiler()
    cfg_cls, _ = _ngp_model_classes()
    base = copy.deepcopy(method_configs["instant-ngp"])
    old = base.pipeline.model
    kwargs = {f.name: getattr(old, f.name) for f in dataclasses.fields(old) if f.name != "_target"}
    base.pipeline.model = cfg_cls(**kwargs)
    # the pipeline whose `get_train_loss_dict` runs the explicit packed-sample schedule with the arena's fused Adam
    # (pipeline.HipDynamicBatchPipeline): DynamicBatchPipelineConfig's fields, another `_target`
    from .pipeline import ngp_pipeline_classes

    pipe_cls, _ = ngp_pipeline_classes()
    old_pipe = base.pipeline
    base.pipeline = pipe_cls(**{f.name: getattr(old_pipe, f.name) for f in dataclasses.fields(old_pipe) if f.name != "_target"})
    base.method_name = "instant-ngp-hip"
    base.mixed_precision = False  # fp32 kernels: no autocast, no loss scaling
    return MethodSpecification(config=base, description=NGP_DESCRIPTION)


def nerfacto_hip():
    """-> MethodSpecification for `ns-train nerfacto-hip`. Raises ImportError when nerfstudio is not importable."""
    import copy
    import dataclasses

    try:
        from nerfstudio.configs.method_configs import method_configs
        from nerfstudio.plugins.types import MethodSpecification
    except Exception as e:  # noqa: BLE001 - tyro / viser / torchmetrics missing count as "nerfstudio not importable"
        raise ImportError(f"nerfstudio_amd.plugin: nerfstudio (with its trainer dependencies) is not importable: {e}") from e
    from .utils import profiler

    profiler.hook_reference_profiler()  # the reference's own time_function hooks open roctx ranges (NSAMD_ROCTX=1)
    cfg_cls, _ = _model_classes()
    base = copy.deepcopy(method_configs["nerfacto"])
    old = base.pipeline.model
    kwargs = {f.name: getattr(old, f.name) for f in dataclasses.fields(old) if f.name not in ("_target", "implementation")}
    base.pipeline.model = cfg_cls(**kwargs)
    # the pipeline whose `get_train_loss_dict` replays the captured training iteration (pipeline.py): same fields as the
    # reference's VanillaPipelineConfig (datamanager, model), another `_target`
    from .pipeline import pipeline_classes

    pipe_cls, _ = pipeline_classes()
    old_pipe = base.pipeline
    base.pipeline = pipe_cls(**{f.name: getattr(old_pipe, f.name) for f in dataclasses.fields(old_pipe) if f.name != "_target"})
    base.method_name = "nerfacto-hip"
    base.mixed_precision = False  # fp32 kernels: no autocast, no loss scaling
    return MethodSpecification(config=base, description=DESCRIPTION)


# nerfstudio's registry loads an ENTRY POINT with `EntryPoint.load()` and keeps it only if the loaded object already IS a
# MethodSpecification (plugins/registry.py:41-51; only the NERFSTUDIO_METHOD_CONFIGS branch calls callables, :64-66). The
# specifications need nerfstudio itself, which this module does not import at import time: they are module attributes
# built on first access (PEP 562) — what pyproject.toml's entry points name.
_LAZY_SPECS = {"nerfacto_hip_spec": nerfacto_hip, "instant_ngp_hip_spec": instant_ngp_hip}


_LAZY_CLASSES = {"HipNerfactoModelConfig": _model_classes, "HipNerfactoModel": _model_classes,
                 "HipInstantNGPModelConfig": _ngp_model_classes, "HipNGPModel": _ngp_model_classes,
                 "HipDepthNerfactoModelConfig": _depth_model_classes, "HipDepthNerfactoModel": _depth_model_classes}


def __getattr__(name: str):
    if name in _LAZY_CLASSES:  # a spawned rank unpickling the TrainerConfig, yaml loading config.yml
        _LAZY_CLASSES[name]()
        return globals()[name]
    builder = _LAZY_SPECS.get(name)
    if builder is None:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    spec = builder()
    globals()[name] = spec
    return spec
