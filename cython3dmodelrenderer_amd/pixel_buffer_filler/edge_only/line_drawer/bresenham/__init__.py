from .line_bresenham import LineBresenham

__all__ = ["LineBresenham"]
