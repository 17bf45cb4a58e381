"""Illuminations of the reference's crender/py: ``GuroIllumination`` on the uint8 colour Buffer (host
and device forms); ``NoIllumination`` and ``IlluminationDrawer`` are the package's own."""
from ...illumination import IlluminationDrawer, NoIllumination
from .guro_illumination import GuroIllumination

__all__ = ["GuroIllumination", "IlluminationDrawer", "NoIllumination"]
