"""Host-side mirror of the reference's supervision/ (the losses of the depth and segmentation training scripts and of view synthesis)."""
from . import chamfer, direct, geometry, photometric, semantic, smoothness, splatting, ssim  # noqa: F401
from .chamfer import chamfer_distance, depth_chamfer, nearest_neighbours  # noqa: F401
from .geometry import geometry_terms, gradient_loss, normal_loss, planefit_normal_loss  # noqa: F401
from .photometric import PhotometricLossParameters, calculate_loss  # noqa: F401
from .semantic import cross_entropy, segmentation_step  # noqa: F401
from .smoothness import depth_smoothness, guided_smoothness_loss  # noqa: F401
from .ssim import ssim_loss  # noqa: F401
