"""mip-NeRF on the MI355X kernels: the wiring of the reference's MipNerfModel (nerfstudio/models/mipnerf.py:57-161) over this
package's modules. It is vanilla_nerf.NeRFModel's render — UniformSampler -> field -> weights -> PDFSampler -> field, white
background, median depth, MSE of both renders — with ONE field for both passes, PDFSampler(include_original=False) and the losses
scaled by the loss coefficients. The field is a NeRFField with integrated positional encoding: each sample is the Gaussian of its
conical frustum, formed from rays and bin edges inside the encoding kernel (csrc/ipe.hip). Temporal distortion and gradient
scaling are not built."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Tuple

from torch.nn import Parameter

from .field_components.encodings import NeRFEncoding
from .fields.vanilla_nerf_field import NeRFField
from .model_components.losses import MSELoss
from .model_components.ray_samplers import PDFSampler, UniformSampler
from .model_components.renderers import AccumulationRenderer, DepthRenderer, RGBRenderer
from .model_components.scene_colliders import NearFarCollider
from .vanilla_nerf import NeRFModel, VanillaModelConfig


@dataclass
class MipNerfModelConfig(VanillaModelConfig):
    """VanillaModelConfig as method_configs["mipnerf"] fills it (configs/method_configs.py): 128 + 128 samples, the coarse
    loss at a tenth (base_model.py:50: `loss_coefficients`, which MipNerfModel applies instead of the two multipliers)."""

    num_coarse_samples: int = 128
    num_importance_samples: int = 128
    loss_coefficients: Dict[str, float] = field(default_factory=lambda: {"rgb_loss_coarse": 0.1, "rgb_loss_fine": 1.0})


class MipNerfModel(NeRFModel):
    """models/mipnerf.py:38-161; `forward`, `get_outputs`, `get_loss_dict` and what is declined are NeRFModel's."""

    config: MipNerfModelConfig
    clip_rgb_for_metrics = True  # models/mipnerf.py:196-197: the image metrics take the predictions clipped to [0, 1]

    def populate_modules(self) -> None:
        position_encoding = NeRFEncoding(in_dim=3, num_frequencies=16, min_freq_exp=0.0, max_freq_exp=16.0, include_input=True)
        direction_encoding = NeRFEncoding(in_dim=3, num_frequencies=4, min_freq_exp=0.0, max_freq_exp=4.0, include_input=True)
        self.field = NeRFField(position_encoding=position_encoding, direction_encoding=direction_encoding,
                               use_integrated_encoding=True)
        self.sampler_uniform = UniformSampler(num_samples=self.config.num_coarse_samples)
        self.sampler_pdf = PDFSampler(num_samples=self.config.num_importance_samples, include_original=False)
        self.renderer_rgb = RGBRenderer(background_color=self.config.background_color)
        self.renderer_accumulation = AccumulationRenderer()
        self.renderer_depth = DepthRenderer()
        self.rgb_loss = MSELoss()
        self.collider = NearFarCollider(near_plane=self.config.near_plane, far_plane=self.config.far_plane)

    def fields(self) -> Tuple[NeRFField, NeRFField]:
        return self.field, self.field

    def get_param_groups(self) -> Dict[str, List[Parameter]]:
        return {"fields": list(self.field.parameters())}

    def loss_scales(self) -> Tuple[float, float]:
        """models/mipnerf.py:160, misc.scale_dict: the loss coefficients; an entry they do not name stays as it is. The two
        multipliers the config inherits are not read, as in the reference."""
        coefficients = self.config.loss_coefficients
        return coefficients.get("rgb_loss_coarse", 1.0), coefficients.get("rgb_loss_fine", 1.0)
