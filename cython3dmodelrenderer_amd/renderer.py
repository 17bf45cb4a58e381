"""Caller of the hot path — mirror of the reference's ``crender.cy.Renderer``
(reference: crender/cy/renderer.py:9-52): optional model fit, ``render_model``,
illumination, return the colour buffer."""
import weakref

import numpy as np


def _device_form_is_the_same_shading(illumination):
    """True if the class that defines ``draw_illumination_device`` is the one that defines
    ``draw_illumination`` (or derives from it): the device form then belongs to the host form in
    force.  A subclass overriding only ``draw_illumination`` makes the inherited device form stale."""
    host_at = dev_at = None
    for i, cls in enumerate(type(illumination).__mro__):
        if host_at is None and "draw_illumination" in vars(cls):
            host_at = i
        if dev_at is None and "draw_illumination_device" in vars(cls):
            dev_at = i
    return dev_at is not None and host_at is not None and dev_at <= host_at


class Renderer:
    def __init__(self, pixel_buffer_filler, illumination, triangle_iterator_type=None,
                 image_height=512, image_width=512, use_tqdm=True, on_device=None, texture_pass=None):
        self.pixel_buffer_filler = pixel_buffer_filler
        self.illumination = illumination
        self.triangle_iterator_type = triangle_iterator_type   # stored, unused (as in Version C)
        self.im_h = image_height
        self.im_w = image_width
        self.use_tqdm = use_tqdm
        # on_device=None (default): same call sequence and same return value as the reference — the
        #   filler's writable numpy colour buffer — but when the filler keeps its buffers on the GPU
        #   and the illumination has a device form, the shading runs there, so that only the colour
        #   plane crosses PCIe (the normals are never handed out);
        # on_device=False: the reference's data flow to the letter, numpy illumination on the
        #   filler's host views of colour and normals;
        # on_device=True: shading on the GPU, returns the colour TENSOR (nothing crosses PCIe);
        # on_device="fused": one model per frame — the frame starts from cleared buffers and the
        #   raster kernel shades each pixel as it stores it (no illumination pass at all).
        self.on_device = on_device
        # texture_pass=None (default): the reference's colours — three vertex colours blended across each triangle.
        # A dict of ``perspective`` / ``filter`` / ``anisotropy`` (AdvancedPixelBufferFiller.texture_pass's arguments;
        # {} = affine, nearest; the filter "trilinear", which ``anisotropy`` above 1 needs, binds the texture with
        # its mip chain): every frame starts from cleared
        # buffers (one model per frame, as "fused") and the model's texture is mapped per pixel before the
        # illumination; with on_device="fused" the texture pass carries the light and the raster kernel does not shade.
        self.texture_pass = None if texture_pass is None else dict(texture_pass)
        self._textured = None          # weak reference to the model whose texture the filler holds

    def _draw(self, model, light=None, **kw):
        """``render_model``; with a texture pass, a cleared frame and the pass on top of it."""
        filler = self.pixel_buffer_filler
        if self.texture_pass is None:
            return filler.render_model(model, **kw)
        if self._textured is None or self._textured() is not model:      # once per model, not per frame
            getters = [getattr(model, n, None) for n in ("get_texture_coords_by_triangles", "get_texture")]
            uv, tex = [g() if g is not None else None for g in getters]
            if uv is None or tex is None:
                raise ValueError("Renderer(texture_pass=...) needs a textured model: this one has no texture "
                                 "coordinates or no texture image")
            if self.texture_pass.get("filter") == "trilinear":
                filler.bind_texture(uv, tex, mipmaps=True)
            else:
                filler.bind_texture(uv, tex)
            self._textured = weakref.ref(model)
        # (the views handed out so far are refreshed by the next getter call, after the pass; and the raster
        # kernel never shades here: the colours it stores are replaced by the texture's)
        filler.set_fused_illumination(None)
        filler.render_model(model, clear=True, refresh_views=False)
        filler.texture_pass(light_direction=light, **self.texture_pass)

    def render(self, model, normalize_model=False, random_colors=True):
        if normalize_model:
            # fit the model into the image (reference: renderer.py:41-46)
            centre = (self.im_h // 2, self.im_w // 2)
            span = min(centre)
            model.scale(span / model.get_max_span())
            model.shift(-model.get_mean_vertex() + [centre[0], centre[1], -span])
        filler = self.pixel_buffer_filler
        if self.on_device == "fused" and getattr(self.illumination, "fuse_into", None):
            if self.texture_pass is not None:
                # the texture pass carries the light
                self._draw(model, light=self.illumination.light_direction)
                return filler.get_color_tensor()
            self.illumination.fuse_into(filler)
            filler.render_model(model, clear=True)
            return filler.get_color_tensor()
        device_form = getattr(self.illumination, "draw_illumination_device", None)
        if self.on_device is None and not _device_form_is_the_same_shading(self.illumination):
            # a subclass that overrides draw_illumination alone — the reference's only hook
            # (renderer.py:47-49) — gets ITS shading, on the host views, not the parent's device form
            device_form = None
        if self.on_device is not False and device_form is not None and hasattr(filler, "get_color_tensor"):
            # (the views handed out so far are refreshed by the getter below, after the shading)
            self._draw(model, refresh_views=False)
            if device_form(filler):
                return filler.get_color_tensor() if self.on_device is True else filler.get_color_buffer()
        else:
            self._draw(model)
        self.illumination.draw_illumination(filler.get_color_buffer(), filler.get_normals_buffer())
        return filler.get_color_buffer()

    def reset_buffers(self):
        pass   # a no-op in the reference too (renderer.py:51-52): renders composite
