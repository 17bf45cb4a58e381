"""The hot path: ``AdvancedPixelBufferFiller`` backed by the HIP library (the reference's
``crender.cy.pixel_buffer_filler``), and the wireframe filler ``EdgeOnlyPixelBufferFiller`` with its
line drawers (``edge_only``; whole meshes drawn by csrc/wireframe.hip)."""
from . import advanced_pixel_buffer_filler as _filler
from .edge_only import EdgeOnlyPixelBufferFiller, LineBresenham, LineDrawer

AdvancedPixelBufferFiller = _filler.AdvancedPixelBufferFiller

__all__ = ["AdvancedPixelBufferFiller", "EdgeOnlyPixelBufferFiller", "LineBresenham", "LineDrawer"]
