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
                 image_height=512, image_width=512, use_tqdm=True, on_device=None, texture_pass=None,
                 shadow=None, ambient_occlusion=None, antialias=None, depth_of_field=None, motion_blur=None, normal_map=None,
                 environment=None, bloom=None, transparency=None, wireframe=None, supersample=None):
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
        # supersample=None (default): the filler's frame is the image.  An int s from 1 to 8: the filler IS the
        # supersampled frame — the caller constructs it at s*H x s*W, and image_height / image_width stay ITS size,
        # so that normalize_model fits the model to the frame actually drawn — and ``render`` returns the mean of
        # every s x s block of it, [H, W, 3] float32, resolved on the device (``filler.resolve``):
        #   "fused"  the raster kernel (or the texture pass) shades as ever, then the resolve; the tensor;
        #   True, or None with an illumination whose device form is its shading and has a ``light_direction``:
        #            the resolve shades each sample as it reads it, there is no illumination pass over the
        #            supersampled planes and the filler's colour plane stays UNSHADED; the tensor for True,
        #            for None a fresh numpy array (a copy: not a live view of a filler plane, edits go nowhere);
        #   False, or an illumination without such a device form: the reference's flow on the host views at
        #            full size, then the resolve (which the edits made there reach); a fresh numpy array.
        # ``filler.resolve(s, light_direction=..., dtype="uint8", flip_rows=True)`` gives the PNG's bytes.
        if supersample is not None and not hasattr(pixel_buffer_filler, "resolve"):
            raise ValueError("Renderer(supersample=...) needs a filler that keeps its planes on the device "
                             "(AdvancedPixelBufferFiller, EdgeOnlyPixelBufferFiller): this one has no resolve()")
        self.supersample = supersample
        # shadow=None (default): no light is occluded.  A dict of ``filler`` (a second AdvancedPixelBufferFiller, the
        # light's: its frame is the shadow map), ``R`` and ``t`` (the light's frame, ``shadow.look_at``) and, optionally,
        # ``bias`` / ``pcf`` / ``ambient`` / ``use_winner`` (AdvancedPixelBufferFiller.shadow_pass's arguments): every
        # frame starts from cleared buffers (one model per frame, as "fused"), the model is drawn a second time from the
        # light, and the shadow pass runs on the camera's frame after any texture pass and before the illumination and
        # the resolve (with on_device="fused" the raster kernel or the texture pass has shaded already: the factors of
        # light and shadow commute up to rounding, the pass multiplies what it finds).
        self.shadow = None
        if shadow is not None:
            if not hasattr(pixel_buffer_filler, "shadow_pass"):
                raise ValueError("Renderer(shadow=...) needs a filler with a shadow pass (AdvancedPixelBufferFiller): "
                                 "this one has no shadow_pass()")
            missing = [k for k in ("filler", "R", "t") if k not in shadow]
            if missing:
                raise ValueError(f"Renderer(shadow=...) needs the keys 'filler', 'R' and 't': {missing} missing")
            self.shadow = dict(shadow)
        # ambient_occlusion=None (default): creases are lit like open surfaces.  A dict of AdvancedPixelBufferFiller.ao_pass's
        # arguments ({} = its defaults): every frame starts from cleared buffers (one model per frame, as "fused") and the
        # pass runs on the camera's frame after any texture pass and BEFORE the Phong pass, the shadow pass, the
        # illumination and the resolve: it scales the surface colour, so Phong's additive highlight is not dimmed.  With
        # on_device="fused" it multiplies what the raster kernel or the texture pass stored; with ``supersample=s`` it
        # runs on the supersampled frame, and ``radius_px`` counts that frame's pixels.
        self.ambient_occlusion = None
        if ambient_occlusion is not None:
            if not hasattr(pixel_buffer_filler, "ao_pass"):
                raise ValueError("Renderer(ambient_occlusion=...) needs a filler with an ambient-occlusion pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no ao_pass()")
            self.ambient_occlusion = dict(ambient_occlusion)
        # wireframe=None (default): no lines.  A dict of AdvancedPixelBufferFiller.wire_pass's arguments ({} = its defaults:
        # every edge, one pixel wide, white) and, optionally, ``feature_angle``: the edge mask is then
        # ``wireframe.feature_edges(the model's triangles, feature_angle)``, computed once per model.  Every frame starts
        # from cleared buffers (one model per frame, as "fused").  The lines are an overlay and are NOT lit: the pass
        # runs after everything that shades — the illumination in whichever form, the shadow pass under a
        # PhongIllumination — and before the resolve.  With ``supersample=s`` it runs on the supersampled frame, ``width``
        # counts that frame's pixels, and the light cannot ride in the resolve (it would shade the lines): the
        # illumination's device form runs over the supersampled frame, then the wire pass, then the plain resolve.
        self.wireframe = None
        self._wired = None             # (weak reference to the model, its feature-edge mask)
        if wireframe is not None:
            if not hasattr(pixel_buffer_filler, "wire_pass"):
                raise ValueError("Renderer(wireframe=...) needs a filler with a wireframe pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no wire_pass()")
            # ``contours`` (True): the edge mask is rebuilt for every frame's view on the device
            # (``AdvancedPixelBufferFiller.contour_edges``) from the model's partner table (``wireframe.edge_partners``,
            # once per model, on the device for a device model): the contour edges, over the ``feature_angle`` mask or
            # an explicit ``edges`` if there is one, and with ``borders`` (default True) the rim of an open mesh.
            if wireframe.get("contours") and not hasattr(pixel_buffer_filler, "contour_edges"):
                raise ValueError("Renderer(wireframe={'contours': True}) needs a filler that classifies contour edges "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no contour_edges()")
            # ``hidden`` (True, or a dict of AdvancedPixelBufferFiller.hidden_line_pass's arguments): the edges BEHIND the
            # surface, dashed, right after the wire pass and with the same mask of the view, so that the contours, creases
            # and borders of the far side are drawn; with ``supersample=s`` on the supersampled frame, whose pixels
            # ``dash`` counts.
            hidden = wireframe.get("hidden")
            if hidden is not None and hidden is not False:
                if not hasattr(pixel_buffer_filler, "hidden_line_pass"):
                    raise ValueError("Renderer(wireframe={'hidden': ...}) needs a filler with a hidden-line pass "
                                     f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no hidden_line_pass()")
                if hidden is not True and not isinstance(hidden, dict):
                    raise ValueError(f"Renderer(wireframe={{'hidden': ...}}) takes True or a dict of hidden_line_pass's "
                                     f"arguments, got {hidden!r}")
            # ``vector`` (True, or a dict of AdvancedPixelBufferFiller.line_runs' arguments): after the wire pass and the
            # hidden pass of a frame the same view's drawing is also taken as vector segments, with the view's mask reduced
            # to one half-edge per edge (``wireframe.half_edges_once``) and the model's partner table (the contours' own, or
            # made once per model), and kept as ``renderer.line_drawing`` (``wireframe.write_svg`` writes it).  With
            # ``supersample=s`` its coordinates are the supersampled frame's.
            vector = wireframe.get("vector")
            if vector is not None and vector is not False:
                if not hasattr(pixel_buffer_filler, "line_runs"):
                    raise ValueError("Renderer(wireframe={'vector': ...}) needs a filler that returns the drawing as vectors "
                                     f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no line_runs()")
                if vector is not True and not isinstance(vector, dict):
                    raise ValueError(f"Renderer(wireframe={{'vector': ...}}) takes True or a dict of line_runs' "
                                     f"arguments, got {vector!r}")
            self.wireframe = dict(wireframe)
        self.line_drawing = None       # the last frame's LineDrawing under wireframe={"vector": ...}
        self._paired = None            # (weak reference to the model, its partner table) where the contours keep none
        # antialias=None (default): every pixel is its one sample.  A dict: geometric edge anti-aliasing
        # (``AdvancedPixelBufferFiller.edge_aa``) of the finished frame — {} smooths every edge, ``edges`` is an explicit
        # mask, and ``feature_angle`` / ``contours`` / ``borders`` pick the edges as ``wireframe`` picks them (the mask
        # and the partner table once per model, the contours of the view every frame).  Every frame starts from cleared
        # buffers (one model per frame, as "fused").  The pass runs LAST, after everything that shades and after the wire
        # pass, reads the filler's planes and writes a tensor of its own, which ``render`` returns: the tensor for
        # on_device=True / "fused", a fresh numpy copy for None / False (as under ``supersample``, with which it does
        # not combine).
        self.antialias = None
        self._smoothed = None          # as _wired, for the edges of ``antialias``
        if antialias is not None:
            if supersample is not None:
                raise ValueError("Renderer(antialias=...) together with supersample=...: the pass smooths the frame's own "
                                 "pixels and does not combine with the resolve; use one of the two")
            if not hasattr(pixel_buffer_filler, "edge_aa"):
                raise ValueError("Renderer(antialias=...) needs a filler with an edge anti-aliasing pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no edge_aa()")
            if antialias.get("contours") and not hasattr(pixel_buffer_filler, "contour_edges"):
                raise ValueError("Renderer(antialias={'contours': True}) needs a filler that classifies contour edges "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no contour_edges()")
            unknown = sorted(set(antialias) - {"edges", "feature_angle", "contours", "borders"})
            if unknown:
                raise ValueError(f"Renderer(antialias=...) takes the keys 'edges', 'feature_angle', 'contours' and "
                                 f"'borders': {unknown} unknown")
            self.antialias = dict(antialias)
        # depth_of_field=None (default): a pinhole image, sharp at every depth.  A dict of
        # ``AdvancedPixelBufferFiller.depth_of_field``'s arguments (``focus``, which it needs, and ``aperture`` / ``band`` /
        # ``max_radius``): a gather blur of the finished frame by every pixel's circle of confusion.  Every frame starts
        # from cleared buffers (one model per frame, as "fused").  The pass runs LAST, after everything that shades and
        # after the wire pass, reads the filler's planes and writes a tensor of its own, which ``render`` returns: the
        # tensor for on_device=True / "fused", a fresh numpy copy otherwise.  It combines neither with ``antialias`` (each
        # of the two reads the filler's colour plane and returns a plane of its own: the second would not see the first)
        # nor with ``supersample`` (the radii would count the supersampled frame's pixels, and the resolve reads the
        # filler's plane, not the pass's).
        self.depth_of_field = None
        if depth_of_field is not None:
            if antialias is not None or supersample is not None:
                raise ValueError("Renderer(depth_of_field=...) together with antialias=... or supersample=...: each of them "
                                 "reads the filler's own colour plane and would not see the blurred one; use one of them")
            if not hasattr(pixel_buffer_filler, "depth_of_field"):
                raise ValueError("Renderer(depth_of_field=...) needs a filler with a depth-of-field pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no depth_of_field()")
            unknown = sorted(set(depth_of_field) - {"focus", "aperture", "band", "max_radius"})
            if unknown:
                raise ValueError("Renderer(depth_of_field=...) takes the keys 'focus', 'aperture', 'band' and 'max_radius': "
                                 f"{unknown} unknown")
            if "focus" not in depth_of_field:
                raise ValueError("Renderer(depth_of_field=...) needs 'focus', the view depth that stays sharp")
            self.depth_of_field = dict(depth_of_field)
        # motion_blur=None (default): every frame is an instant.  A dict of ``exposure`` / ``max_radius`` / ``taps`` / ``soft``
        # (``AdvancedPixelBufferFiller.motion_blur``'s arguments; {} = its defaults): the finished frame blurred along the
        # motion vectors of the model between the pose of the ``render`` call before and this one's.  At every ``render``
        # the renderer keeps a device COPY of the vertex array the frame was drawn from (a DeviceModel is transformed in
        # place) and uses the copy of the call before as the previous pose; on the first call, after ``reset_motion()``
        # and when the triangle count changed, the previous pose is the current one and the image is the frame, copied.
        # Every frame starts from cleared buffers (one model per frame, as "fused").  The pass runs LAST, after everything
        # that shades and after the wire pass, reads the filler's planes and writes a tensor of its own, which ``render``
        # returns (``bloom`` reads it): the tensor for on_device=True / "fused", a fresh numpy copy otherwise.  It combines
        # with none of ``antialias``, ``depth_of_field``, ``supersample`` and ``transparency``: each of them reads the
        # filler's own colour plane and would not see the blurred one.
        self.motion_blur = None
        self._previous_pose = None     # the device copy of the vertices the last frame was drawn from
        if motion_blur is not None:
            if antialias is not None or depth_of_field is not None or supersample is not None or transparency is not None:
                raise ValueError("Renderer(motion_blur=...) together with antialias=..., depth_of_field=..., supersample=... or "
                                 "transparency=...: each of them reads the filler's own colour plane and would not see the "
                                 "blurred one; use one of them")
            if not hasattr(pixel_buffer_filler, "motion_blur"):
                raise ValueError("Renderer(motion_blur=...) needs a filler with a motion-blur pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no motion_blur()")
            unknown = sorted(set(motion_blur) - {"exposure", "max_radius", "taps", "soft"})
            if unknown:
                raise ValueError("Renderer(motion_blur=...) takes the keys 'exposure', 'max_radius', 'taps' and 'soft': "
                                 f"{unknown} unknown")
            self.motion_blur = dict(motion_blur)
        # normal_map=None (default): the light sees the interpolated vertex normals.  A dict of
        # AdvancedPixelBufferFiller.bind_normal_map's arguments but the uv (``normal_map`` or ``height``, ``scale``, ``wrap``,
        # ``mipmaps``) and of normal_map_pass's (``strength``, ``perspective``, ``filter``; "trilinear" binds the map with
        # its mip chain): the map is bound here, once, and the model's texture coordinates once per model.  Every frame
        # starts from cleared buffers (one model per frame, as "fused") and the pass runs FIRST, directly after the draw:
        # it perturbs the normal plane, which the ambient occlusion, the fused light of the texture pass, the Phong
        # pass, the illumination and the resolve read afterwards.  With ``supersample=s`` it runs on the supersampled
        # frame.  on_device="fused" needs a ``texture_pass`` (which then carries the light): without one the raster
        # kernel has shaded from the unperturbed normals before any pass can run.
        self.normal_map = None
        self._bumped = None            # weak reference to the model whose uv the normal map is bound with
        if normal_map is not None:
            if not hasattr(pixel_buffer_filler, "normal_map_pass"):
                raise ValueError("Renderer(normal_map=...) needs a filler with a normal-map pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no normal_map_pass()")
            if on_device == "fused" and texture_pass is None:
                raise ValueError("Renderer(normal_map=..., on_device='fused') without a texture_pass: the raster kernel "
                                 "shades from the unperturbed normals before any pass can run; add a texture_pass, which "
                                 "carries the light, or use another on_device")
            opts = dict(normal_map)
            unknown = sorted(set(opts) - {"normal_map", "height", "scale", "wrap", "mipmaps", "strength", "perspective", "filter"})
            if unknown:
                raise ValueError("Renderer(normal_map=...) takes the keys 'normal_map', 'height', 'scale', 'wrap', 'mipmaps', "
                                 f"'strength', 'perspective' and 'filter': {unknown} unknown")
            self.normal_map = {k: opts.pop(k) for k in ("strength", "perspective", "filter") if k in opts}
            if self.normal_map.get("filter") == "trilinear":
                opts.setdefault("mipmaps", True)
            pixel_buffer_filler.bind_normal_map(opts.pop("normal_map", None), **opts)
            if pixel_buffer_filler.get_normal_map() is None:
                raise ValueError("Renderer(normal_map=...) needs 'normal_map' or 'height'")
        # environment=None (default): nothing is mirrored and the background keeps the cleared colour.  A dict of ``faces``
        # (the cube map, uint8 [6, S, S, 3]: ``environment.cube_from_equirect`` / ``gradient_sky``) and, optionally,
        # ``mipmaps`` (AdvancedPixelBufferFiller.bind_environment's arguments) and ``reflectivity`` / ``f0`` / ``tint`` /
        # ``level`` / ``orientation`` / ``background`` (environment_pass's; a ``level`` above 0 binds the cube with its mip
        # chain): the cube is bound here, once.  Every frame starts from cleared buffers (one model per frame, as "fused")
        # and the pass runs AFTER the light in whichever form — the illumination's device or host form, the fused light
        # of the raster kernel or the texture pass, the Phong pass and its shadow pass — and immediately BEFORE the wire
        # pass, so that the lines and ``antialias`` come after it and silhouettes blend against the sky.  (The sky cannot
        # come before the light: the illumination multiplies the background by the factor of a zero normal.)  With
        # ``supersample=s`` it runs on the supersampled frame and the light cannot ride in the resolve (it would shade
        # the mirror image and the sky): as under ``wireframe``, the light runs as a pass of its own, then the
        # environment, then the wire pass, then the plain resolve.
        self.environment = None
        if environment is not None:
            if not hasattr(pixel_buffer_filler, "environment_pass"):
                raise ValueError("Renderer(environment=...) needs a filler with an environment pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no environment_pass()")
            opts = dict(environment)
            known = ("faces", "mipmaps", "reflectivity", "f0", "tint", "level", "orientation", "background")
            unknown = sorted(set(opts) - set(known))
            if unknown:
                raise ValueError("Renderer(environment=...) takes the keys " + ", ".join(repr(k) for k in known[:-1]) +
                                 f" and {known[-1]!r}: {unknown} unknown")
            if opts.get("faces") is None:
                raise ValueError("Renderer(environment=...) needs 'faces'")
            level = opts.get("level", 0.0)
            if not isinstance(level, bool) and isinstance(level, (int, float, np.integer, np.floating)) and level > 0:
                opts.setdefault("mipmaps", True)
            pixel_buffer_filler.bind_environment(opts.pop("faces"), mipmaps=bool(opts.pop("mipmaps", False)))
            self.environment = opts
        # A PhongIllumination is a deferred pass of the filler over its winner plane (``phong_pass``): every frame
        # starts from cleared buffers (one model per frame, as "fused"); the draw, then the texture pass (unlit) if
        # asked for, then the Phong pass, then the shadow pass — AFTER the light here, since the specular term is
        # additive and a factor applied before it would leave highlights inside shadows: the shadow's ``ambient`` is
        # the floor of everything — then the plain resolve.  None returns the numpy colour view (with supersample a
        # fresh numpy copy), True the tensor.
        from .illumination.phong_illumination import PhongIllumination
        self._phong = isinstance(illumination, PhongIllumination)
        if self._phong:
            if on_device is False or on_device == "fused":
                raise ValueError(f"Renderer(on_device={on_device!r}) with a PhongIllumination: the model needs the winner "
                                 "plane and the triangles, so it has no host form on two planes and is not fused into "
                                 "the raster kernel; use on_device=None or True")
            if not hasattr(pixel_buffer_filler, "phong_pass"):
                raise ValueError("Renderer with a PhongIllumination needs a filler with a Phong pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no phong_pass()")
        # transparency=None (default): every pixel shows its nearest surface and nothing behind it.  A dict of
        # ``AdvancedPixelBufferFiller.transparency_pass``'s arguments (``alpha``, which it needs, and ``layers`` /
        # ``background`` / ``front``): the frame's depth layers peeled and blended front to back.  Every frame starts from
        # cleared buffers (one model per frame, as "fused").  The pass runs LAST, after everything that shades and after the
        # wire pass, reads the filler's planes and writes a tensor of its own, which ``render`` returns: the tensor for
        # on_device=True / "fused", a fresh numpy copy otherwise.  The layers behind the first are lit by the
        # ``light_direction`` of a GuroIllumination (or the key of that name); a PhongIllumination is refused, since they would be lit by another
        # model than the first.  It combines with none of ``antialias``, ``depth_of_field`` and ``supersample``.
        self.transparency = None
        if transparency is not None:
            if antialias is not None or depth_of_field is not None or supersample is not None:
                raise ValueError("Renderer(transparency=...) together with antialias=..., depth_of_field=... or supersample=...: "
                                 "each of them reads the filler's own colour plane and would not see the blended one; use one "
                                 "of them")
            if not hasattr(pixel_buffer_filler, "transparency_pass"):
                raise ValueError("Renderer(transparency=...) needs a filler with a transparency pass "
                                 f"(AdvancedPixelBufferFiller): {type(pixel_buffer_filler).__name__} has no transparency_pass()")
            if self._phong:
                raise ValueError("Renderer(transparency=...) with a PhongIllumination: the layers behind the first are shaded "
                                 "with the Guro light or none and would be lit by another model than the first; use a "
                                 "GuroIllumination")
            unknown = sorted(set(transparency) - {"alpha", "layers", "light_direction", "background", "front"})
            if unknown:
                raise ValueError("Renderer(transparency=...) takes the keys 'alpha', 'layers', 'light_direction', 'background' "
                                 f"and 'front': {unknown} unknown")
            if "alpha" not in transparency:
                raise ValueError("Renderer(transparency=...) needs 'alpha', a number or one value per triangle")
            self.transparency = dict(transparency)
        # bloom=None (default): what is brighter than 255 stays as the frame holds it.  A dict of the filler's ``bloom``
        # arguments but ``source`` ({} = its defaults: a glow of radius 8 around what exceeds 255): bloom and tone mapping
        # of the finished image.  It runs after EVERYTHING else and reads a source: the tensor of ``transparency``,
        # ``depth_of_field``, ``antialias`` or ``supersample``, whichever ran, or else the filler's colour plane — so it
        # combines with each of the four, and alone it changes nothing about how the frame is drawn.  ``render`` returns
        # the pass's own tensor for on_device=True / "fused", a fresh numpy copy otherwise.
        self.bloom = None
        if bloom is not None:
            if not hasattr(pixel_buffer_filler, "bloom"):
                raise ValueError("Renderer(bloom=...) needs a filler that keeps its planes on the device "
                                 "(AdvancedPixelBufferFiller, EdgeOnlyPixelBufferFiller): "
                                 f"{type(pixel_buffer_filler).__name__} has no bloom()")
            from .bloom import KEYS
            unknown = sorted(set(bloom) - set(KEYS))
            if unknown:
                raise ValueError("Renderer(bloom=...) takes the keys " + ", ".join(repr(k) for k in KEYS[:-1]) +
                                 f" and {KEYS[-1]!r}: {unknown} unknown")
            self.bloom = dict(bloom)

    def _draw(self, model, light=None, shadows=True, **kw):
        """``render_model``; with a texture pass, ambient occlusion, a shadow map, an environment or a wireframe, a cleared
        frame and the passes on top of it (but the environment's and the wireframe's, which follow the light:
        ``_draw_wire``)."""
        filler = self.pixel_buffer_filler
        if self.texture_pass is None:
            if self.shadow is None and self.ambient_occlusion is None and self.wireframe is None and self.antialias is None \
                    and self.normal_map is None and self.environment is None and self.depth_of_field is None \
                    and self.transparency is None and self.motion_blur is None:
                return filler.render_model(model, **kw)
            if not kw.get("clear"):        # (the "fused" caller asks for the cleared frame itself: its raster kernel shades)
                filler.set_fused_illumination(None)
            filler.render_model(model, clear=True, refresh_views=False)
            self._bump(model)
            if self.ambient_occlusion is not None:
                filler.ao_pass(**self.ambient_occlusion)
            if self.shadow is not None:
                self._cast_shadows(model)
            return None
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
        self._bump(model)              # before the texture pass, whose fused light reads the normal plane
        filler.texture_pass(light_direction=light, **self.texture_pass)
        if self.ambient_occlusion is not None:
            filler.ao_pass(**self.ambient_occlusion)
        if self.shadow is not None and shadows:
            self._cast_shadows(model)

    def _bump(self, model):
        """The normal-map pass over the frame just drawn, if a normal map was asked for: first of all passes."""
        if self.normal_map is None:
            return
        if self._bumped is None or self._bumped() is not model:          # once per model, not per frame
            getter = getattr(model, "get_texture_coords_by_triangles", None)
            uv = getter() if getter is not None else None
            if uv is None:
                raise ValueError("Renderer(normal_map=...) needs a model with texture coordinates: this one has none")
            self.pixel_buffer_filler.bind_normal_map_uv(uv)
            self._bumped = weakref.ref(model)
        self.pixel_buffer_filler.normal_map_pass(**self.normal_map)

    def _cast_shadows(self, model):
        """The model again, from the light, into the light's filler; then the shadow pass over the camera's frame."""
        from . import shadow
        from .pixel_buffer_filler.advanced_pixel_buffer_filler import _model_arrays
        opts = dict(self.shadow)
        light_filler, R, t = opts.pop("filler"), opts.pop("R"), opts.pop("t")
        tri, col, nrm = _model_arrays(model)
        ltri, lnrm = shadow.light_arrays(tri, nrm, R, t)
        light_filler.render_arrays(ltri, col, lnrm, clear=True)
        self.pixel_buffer_filler.bind_shadow_map(light_filler, ltri)
        self.pixel_buffer_filler.shadow_pass(**opts)

    def _draw_wire(self, model):
        """The environment pass, if one was asked for, and then the wire pass, if a wireframe was, over the frame as it
        stands (host edits included)."""
        if self.environment is not None:
            self.pixel_buffer_filler.environment_pass(**self.environment)
        if self.wireframe is None:
            return
        opts = self._view_edges(model, self.wireframe, "_wired")
        hidden = opts.pop("hidden", None)
        vector = opts.pop("vector", None)
        self.pixel_buffer_filler.wire_pass(**opts)
        if hidden is not None and hidden is not False:
            # right after the visible lines (a ``fill`` would paint over dashes drawn first), with the same mask of the view
            more = {} if hidden is True else dict(hidden)
            more.setdefault("edges", opts.get("edges"))
            self.pixel_buffer_filler.hidden_line_pass(**more)
        if vector is not None and vector is not False:
            # the same view as vectors: every drawn edge once, either of its two triangles makes it visible
            from .wireframe import half_edges_once
            more = {} if vector is True else dict(vector)
            if more.get("partners") is None:
                more["partners"] = self._partners(model)
            if "edges" not in more:
                more["edges"] = half_edges_once(opts.get("edges"), more["partners"])
            self.line_drawing = self.pixel_buffer_filler.line_runs(**more)

    def _partners(self, model):
        """The model's partner table: the one the contours of ``wireframe`` hold, or one made once per model."""
        if self._wired is not None and self._wired[0]() is model and self._wired[2] is not None:
            return self._wired[2]
        if self._paired is None or self._paired[0]() is not model:
            from .wireframe import edge_partners
            partners = edge_partners(model._vertices_by_triangles)      # (a device model's table is made on the device)
            device = getattr(self.pixel_buffer_filler, "device", None)
            if device is not None and not hasattr(partners, "data_ptr"):
                import torch
                partners = torch.from_numpy(partners).to(device)
            self._paired = (weakref.ref(model), partners)
        return self._paired[1]

    def _view_edges(self, model, options, slot):
        """`options` (``wireframe``'s or ``antialias``'s) with ``feature_angle`` / ``contours`` / ``borders`` turned into
        the ``edges`` of this frame's view.  `slot` names the once-per-model cache, (weak reference to the model, mask,
        partner table, angle); what the other option's cache holds for the same model is taken from there."""
        opts = dict(options)
        angle = opts.pop("feature_angle", None)
        contours, borders = opts.pop("contours", False), opts.pop("borders", True)
        if angle is not None or contours:
            cache = getattr(self, slot)
            if cache is None or cache[0]() is not model:     # once per model, not per frame
                from .wireframe import edge_partners, feature_edges
                other = self._smoothed if slot == "_wired" else self._wired
                if other is not None and other[0]() is not model:
                    other = None
                tri = model._vertices_by_triangles
                device = getattr(self.pixel_buffer_filler, "device", None)
                mask = partners = None
                if angle is not None:
                    if other is not None and other[1] is not None and other[3] == angle:
                        mask = other[1]
                    else:
                        mask = feature_edges(tri.cpu().numpy() if hasattr(tri, "cpu") else tri, angle)
                        if device is not None:
                            import torch
                            mask = torch.from_numpy(mask).to(device)
                if contours:
                    if other is not None and other[2] is not None:
                        partners = other[2]
                    else:
                        partners = edge_partners(tri)      # (a device model's table is made on the device)
                        if device is not None and not hasattr(partners, "data_ptr"):
                            import torch
                            partners = torch.from_numpy(partners).to(device)
                cache = (weakref.ref(model), mask, partners, angle)
                setattr(self, slot, cache)
            if angle is not None:
                opts["edges"] = cache[1]
        if contours:
            # the mask of this frame's view: the contours, over the static mask if there is one
            opts["edges"] = self.pixel_buffer_filler.contour_edges(cache[2], static=opts.get("edges"), borders=bool(borders))
        return opts

    def render(self, model, normalize_model=False, random_colors=True):
        if normalize_model:
            # fit the model into the image (reference: renderer.py:41-46)
            centre = (self.im_h // 2, self.im_w // 2)
            span = min(centre)
            model.scale(span / model.get_max_span())
            model.shift(-model.get_mean_vertex() + [centre[0], centre[1], -span])
        if self.transparency is not None:
            # the frame as ever, then its layers blended, last of all: the pass's own tensor is the image
            self._render(model)
            opts = dict(self.transparency)
            opts.setdefault("light_direction", getattr(self.illumination, "light_direction", None))
            image = self.pixel_buffer_filler.transparency_pass(**opts)
        elif self.depth_of_field is not None:
            # the frame as ever, then the lens, last of all: the pass's own tensor is the image
            self._render(model)
            image = self.pixel_buffer_filler.depth_of_field(**self.depth_of_field)
        elif self.motion_blur is not None:
            # the frame as ever, then the shutter, last of all: the pass's own tensor is the image
            self._render(model)
            image = self._shutter(model)
        elif self.antialias is not None:
            # the frame as ever, then the edges smoothed, last of all: the pass's own tensor is the image
            self._render(model)
            image = self.pixel_buffer_filler.edge_aa(**self._view_edges(model, self.antialias, "_smoothed"))
        else:
            image = self._render(model)
            if self.bloom is None:
                return image
            if self.supersample is None:
                image = None           # the filler's own colour plane, host edits included: bloom completes it itself
        if self.bloom is not None:
            # after everything else: over the tensor of the pass that ran last, or over the filler's plane
            image = self.pixel_buffer_filler.bloom(source=image, **self.bloom)
        return image if self.on_device is True or self.on_device == "fused" else image.cpu().numpy()

    def _render(self, model):
        """``render`` after the model fit: the draws, the light and the passes, in the constructor's order."""
        filler = self.pixel_buffer_filler
        if self._phong:
            return self._render_phong(model)
        if self.supersample is not None:
            return self._render_supersampled(model)
        if self.on_device == "fused" and getattr(self.illumination, "fuse_into", None):
            if self.texture_pass is not None:
                # the texture pass carries the light
                self._draw(model, light=self.illumination.light_direction)
                self._draw_wire(model)
                return filler.get_color_tensor()
            self.illumination.fuse_into(filler)
            self._draw(model, clear=True)
            self._draw_wire(model)
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
                self._draw_wire(model)
                return filler.get_color_tensor() if self.on_device is True else filler.get_color_buffer()
        else:
            self._draw(model)
        self.illumination.draw_illumination(filler.get_color_buffer(), filler.get_normals_buffer())
        self._draw_wire(model)         # (carries the host edits to the device; the view shows the lines)
        return filler.get_color_buffer()

    def _render_phong(self, model):
        """``render`` after the model fit, with a ``PhongIllumination``: the passes in the constructor's order."""
        filler = self.pixel_buffer_filler
        if self.texture_pass is not None:
            self._draw(model, shadows=False)               # the texture, unlit
        else:
            filler.set_fused_illumination(None)
            filler.render_model(model, clear=True, refresh_views=False)
            self._bump(model)
            if self.ambient_occlusion is not None:
                filler.ao_pass(**self.ambient_occlusion)
        self.illumination.draw_illumination_device(filler)
        if self.shadow is not None:
            self._cast_shadows(model)
        self._draw_wire(model)
        if self.supersample is not None:
            image = filler.resolve(self.supersample)
            return image if self.on_device is True or self.bloom is not None else image.cpu().numpy()
        return filler.get_color_tensor() if self.on_device is True else filler.get_color_buffer()

    def _render_supersampled(self, model):
        """``render`` after the model fit, with ``supersample=s``: the same draws, the resolve at the end."""
        filler, s = self.pixel_buffer_filler, self.supersample
        if self.on_device == "fused" and getattr(self.illumination, "fuse_into", None):
            if self.texture_pass is not None:
                self._draw(model, light=self.illumination.light_direction)
            else:
                self.illumination.fuse_into(filler)
                self._draw(model, clear=True)
            self._draw_wire(model)
            return filler.resolve(s)
        light = getattr(self.illumination, "light_direction", None)
        device_form = getattr(self.illumination, "draw_illumination_device", None)
        if self.on_device is None and not _device_form_is_the_same_shading(self.illumination):
            device_form = None
        if self.on_device is not False and device_form is not None and light is not None:
            # the resolve carries the light: the supersampled colour plane is read once and stays unshaded
            self._draw(model, refresh_views=False)
            if self.wireframe is None and self.environment is None:
                image = filler.resolve(s, light_direction=light)
            else:
                # the lines, the mirror image and the sky are not lit: the light as a pass of its own over the supersampled
                # frame, then the environment and the lines
                if not device_form(filler):
                    self.illumination.draw_illumination(filler.get_color_buffer(), filler.get_normals_buffer())
                self._draw_wire(model)
                image = filler.resolve(s)
            return image if self.on_device is True or self.bloom is not None else image.cpu().numpy()
        self._draw(model)
        self.illumination.draw_illumination(filler.get_color_buffer(), filler.get_normals_buffer())
        self._draw_wire(model)
        image = filler.resolve(s)
        return image if self.bloom is not None else image.cpu().numpy()      # (bloom reads the resolve's tensor)

    def _shutter(self, model):
        """The motion-blur pass over the frame just drawn, against the pose of the call before; keeps this call's pose."""
        import torch
        v = model._vertices_by_triangles
        device = getattr(self.pixel_buffer_filler, "device", None)
        if isinstance(v, torch.Tensor):
            current = v.detach().to(device=v.device if device is None else device, copy=True)
        else:
            current = torch.from_numpy(np.array(v, copy=True))
            if device is not None:
                current = current.to(device)
        previous = self._previous_pose
        if previous is None or previous.shape[0] != current.shape[0]:
            previous = current         # a static pose: the frame, copied
        self._previous_pose = current
        return self.pixel_buffer_filler.motion_blur(previous, **self.motion_blur)

    def reset_motion(self):
        """Forget the previous pose: the next ``render`` under ``motion_blur`` returns its frame unblurred (a camera cut)."""
        self._previous_pose = None

    def reset_buffers(self):
        pass   # a no-op in the reference too (renderer.py:51-52): renders composite
