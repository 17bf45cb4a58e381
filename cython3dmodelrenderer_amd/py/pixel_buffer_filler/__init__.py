"""Fillers of the reference's crender/py: the numpy ``AdvancedPixelBufferFiller`` (uint8 colour plane,
whole sequences drawn by csrc/pyfill.hip) and, re-exported, the wireframe ``EdgeOnlyPixelBufferFiller``."""
from ...pixel_buffer_filler.edge_only import EdgeOnlyPixelBufferFiller
from .advanced_pixel_buffer_filler import AdvancedPixelBufferFiller

__all__ = ["AdvancedPixelBufferFiller", "EdgeOnlyPixelBufferFiller"]
