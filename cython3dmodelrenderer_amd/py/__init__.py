"""The reference's numpy path, ``crender.py``: ``Renderer`` driving a filler with a triangle iterator
onto three ``Buffer`` planes (colour uint8, z float32, normals float32).  The numpy
``AdvancedPixelBufferFiller`` draws whole sequences on the GPU (csrc/pyfill.hip)."""
from .. import triangle_iterator
from . import data_structures, illumination, pixel_buffer_filler
from .renderer import Renderer

__all__ = ["Renderer", "data_structures", "illumination", "pixel_buffer_filler", "triangle_iterator"]
