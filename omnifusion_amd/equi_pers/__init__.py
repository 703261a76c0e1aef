from .equi2pers_v3 import equi2pers  # noqa: F401
from .pers2equi_v3 import pers2equi, pers2equi_conf  # noqa: F401
from ._freeview import cubemap_views, views_to_erp  # noqa: F401
from . import differentiable  # noqa: F401  (the free-view operators with a backward)
