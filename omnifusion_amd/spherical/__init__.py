"""Host-side mirror of /root/reference/spherical/ (the grids DIBR reads)."""
from .grid import create_image_grid, create_spherical_grid  # noqa: F401
