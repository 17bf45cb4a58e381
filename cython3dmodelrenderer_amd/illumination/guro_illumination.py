"""Gouraud-style ("Guro") directional shading, SURVEY.md section 8f row f1
(reference: crender/cy/illumination/guro_illumination.py:6-27):

    colour *= clip(n . l / (|n| + 1e-6), 0, 1)      per pixel, float32, in place

``draw_illumination`` is the numpy form on host arrays (same call sequence as the
reference, so the same bits); ``draw_illumination_device`` has the filler run the HIP kernel
``crender_guro_illumination`` on its device buffers (``shade_guro`` of
pixel_buffer_filler/_device_planes.py, which also keeps the host views right); ``fuse_into`` hands the light
to the filler, whose cleared frames then shade each pixel as the raster kernel stores it
(CRENDER_FUSED_GURO: no second pass over the colour and normal planes).
"""
import numpy as np

from .illumination_drawer import IlluminationDrawer


class GuroIllumination(IlluminationDrawer):
    def __init__(self, light_direction=(0, 0, 1)):
        # the light vector is flipped so that it opposes front-facing normals
        flipped = -np.asarray(light_direction, dtype="float32")
        self.light_direction = flipped / np.linalg.norm(flipped)

    def draw_illumination(self, color_buffer, n_buffer):
        cos = np.sum(n_buffer * self.light_direction, axis=-1, keepdims=True)
        length = np.linalg.norm(n_buffer, axis=-1, keepdims=True)
        color_buffer *= np.clip(cos / (length + 1e-6), 0, 1)

    def draw_illumination_device(self, filler):
        light = [float(v) for v in self.light_direction]      # (before the wait, not after it)
        filler._push_host_edits()
        filler.synchronize()      # the frame must be complete (bin lists may grow and redo it)
        filler.shade_guro(light)
        return True

    def fuse_into(self, filler):
        filler.set_fused_illumination(self.light_direction)
        return True
