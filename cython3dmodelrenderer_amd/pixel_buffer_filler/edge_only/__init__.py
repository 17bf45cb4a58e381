"""Wireframe filler (the reference's ``crender.py.pixel_buffer_filler.edge_only``)."""
from .edge_only_pixel_buffer_filler import EdgeOnlyPixelBufferFiller
from .line_drawer import LineBresenham, LineDrawer

__all__ = ["EdgeOnlyPixelBufferFiller", "LineBresenham", "LineDrawer"]
