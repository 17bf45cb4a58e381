"""The py ``Renderer`` of the reference (crender/py/renderer.py): a filler, an illumination and a triangle
iterator type over three ``Buffer`` planes — colour uint8 [H][W][3] from 0, z float32 [H][W][1] from
1e6, normals float32 [H][W][3] from 0 — onto which ``render`` composites until ``reset_buffers``.

``render`` gives a model without colours its colours on the host first, in iterator order, from the
global numpy RNG (one ``randint(256, size=(T, 3))``: the stream of T calls of ``randint(256,
size=3)``), or white with ``random_colors=False``.  A filler with ``draw_sequence`` (the py
``AdvancedPixelBufferFiller``) then draws every triangle in one GPU call — in the order of the
iterator's ``draw_order`` hook for ``SimpleIterator`` and ``DepthIterator`` on a model with the
``*_by_triangles`` arrays, any other iterator or model drained on the host first — and a py
``GuroIllumination`` is applied on the device before the planes come back.  Any other filler
(``EdgeOnlyPixelBufferFiller``, a custom one) is called once per triangle.
"""
from __future__ import annotations

import numpy as np

from ..triangle_iterator import DepthIterator, SimpleIterator
from .data_structures import Buffer
from .illumination import GuroIllumination

_ARRAYS = ("_vertices_by_triangles", "_colors_by_triangles", "_normals_by_triangles")


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


def _stack(parts, empty):
    return np.stack(parts) if parts else empty


class Renderer:
    def __init__(self, pixel_buffer_filler, illumination, triangle_iterator_type: type,
                 image_height: int = 512, image_width: int = 512, use_tqdm=True):
        self.pixel_buffer_filler, self.illumination = pixel_buffer_filler, illumination
        self.triangle_iterator_type = triangle_iterator_type
        self.im_h, self.im_w = image_height, image_width
        self.use_tqdm = use_tqdm
        self.color_buffer = Buffer(image_height, image_width, dim=3, dtype='uint8')
        self.z_buffer = Buffer(image_height, image_width, dim=1, dtype='float32', init_val=1e6)
        self.n_buffer = Buffer(image_height, image_width, dim=3, dtype='float32')

    def reset_buffers(self):
        for plane in (self.color_buffer, self.z_buffer, self.n_buffer):
            plane.clear()

    def render(self, model, normalize_model=False, random_colors=True):
        """Draw ``model`` onto the buffers, illuminate them and return the colour ``Buffer``.
        ``normalize_model`` first moves and scales the model (in place) into the frame."""
        if normalize_model:
            half_h, half_w = self.im_h // 2, self.im_w // 2
            radius = min(half_h, half_w)
            model.scale(radius / model.get_max_span())
            model.shift(-model.get_mean_vertex() + [half_h, half_w, -radius])
        if hasattr(self.pixel_buffer_filler, "draw_sequence"):
            self._draw_device(model, random_colors)
        else:
            self._draw_per_triangle(model, random_colors)
        return self.color_buffer

    @staticmethod
    def _one_colour(random_colors):
        """The per-corner colours of one triangle without any: one draw of the global RNG, or white."""
        rgb = np.random.randint(256, size=3) if random_colors else np.full(3, 255)
        return np.tile(rgb, (3, 1))

    def _draw_per_triangle(self, model, random_colors):
        triangles = self.triangle_iterator_type(model)
        if self.use_tqdm:
            from tqdm import tqdm
            triangles = tqdm(triangles)
        fill = self.pixel_buffer_filler.compute_triangle_statistics
        for vertices, colours, normals in triangles:
            if colours is None:
                colours = self._one_colour(random_colors)
            fill(vertices, colours, normals, self.color_buffer, self.z_buffer, self.n_buffer)
        self.illumination.draw_illumination(self.color_buffer, self.n_buffer)

    def _ordered_arrays(self, model):
        """(vertices, colours or None, normals) [T, 3, 3] in iterator order."""
        kind = self.triangle_iterator_type
        if kind in (SimpleIterator, DepthIterator) and all(hasattr(model, a) for a in _ARRAYS):
            tri, col, nrm = (_host(getattr(model, a)) for a in _ARRAYS)
            perm = kind.draw_order(model)
            if perm is not None:
                tri, nrm = np.asarray(tri)[perm], np.asarray(nrm)[perm]
                col = None if col is None else np.asarray(col)[perm]
            return tri, col, nrm
        items = list(kind(model))
        tri = _stack([np.asarray(v) for v, _, _ in items], np.zeros((0, 3, 3), np.float32))
        nrm = _stack([np.asarray(n) for _, _, n in items], np.zeros((0, 3, 3), np.float32))
        col = None if not items or items[0][1] is None else np.stack([c for _, c, _ in items])
        return tri, col, nrm

    def _draw_device(self, model, random_colors):
        tri, col, nrm = self._ordered_arrays(model)
        if col is None:
            count = len(tri)
            rgb = np.random.randint(256, size=(count, 3)) if random_colors else np.full((count, 3), 255)
            col = np.repeat(rgb[:, None, :], 3, axis=1)
        light = self.illumination.light_direction if type(self.illumination) is GuroIllumination else None
        self.pixel_buffer_filler.draw_sequence(tri, col, nrm, self.color_buffer, self.z_buffer, self.n_buffer,
                                               light=light)
        if light is None:
            self.illumination.draw_illumination(self.color_buffer, self.n_buffer)
