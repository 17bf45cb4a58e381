from .line_drawer import LineDrawer
from .bresenham import LineBresenham

__all__ = ["LineDrawer", "LineBresenham"]
