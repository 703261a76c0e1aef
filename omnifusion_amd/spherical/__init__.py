"""Host-side mirror of the reference's spherical/ (the grids DIBR reads, the vertices, derivatives and weights of the smoothness term)."""
from . import cartesian, derivatives, grid, weights  # noqa: F401
from .cartesian import coord_x, coord_y, coord_z, coords_3d, xi, yi, zeta  # noqa: F401
from .derivatives import dI_du, dI_duv, dI_dv, dV_dx, dV_dxyz, dV_dy, dV_dz  # noqa: F401
from .grid import (azimuth, create_image_grid, create_spherical_grid, elevation, latitude, longitude, phi, theta)  # noqa: F401
from .weights import phi_confidence, spherical_confidence, theta_confidence  # noqa: F401
