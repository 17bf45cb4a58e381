"""Caller of the hot path — mirror of the reference's ``crender.cy.Renderer``
(reference: crender/cy/renderer.py:9-52): optional model fit, ``render_model``,
illumination, return the colour buffer."""
import weakref
from collections import namedtuple

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


def _bloom_keys():
    from .bloom import KEYS
    return KEYS


# What the constructor checks of one option, in this order: `excludes`, the options it does not combine with (`clash`
# is the refusal's text); `method`, what the filler must have (`needs` names it in the refusal: "... needs a filler
# <needs> has no <method>()", {filler} in it is the filler's type); the option's own checks (``Renderer.__init__``);
# `known`, the keys it takes (None: they are passed through; a function where they are imported late); `required`,
# the keys it must have (`missing` is the refusal's text).  `clears`: every frame starts from cleared buffers (one
# model per frame, as on_device="fused").
_Option = namedtuple("_Option", "name method needs known required missing excludes clash clears",
                     defaults=(None, (), "", (), "", True))
_PASS = "(AdvancedPixelBufferFiller): {filler}"
_OWN_PLANE = "each of them reads the filler's own colour plane and would not see the "

# One record per option of ``Renderer``, in the order in which the constructor checks them; the comment of each says
# what the option is and where its pass runs in a frame.
_OPTIONS = (
    # texture_pass=None (default): the reference's colours — three vertex colours blended across each triangle.
    # A dict of ``perspective`` / ``filter`` / ``anisotropy`` (AdvancedPixelBufferFiller.texture_pass's arguments;
    # {} = affine, nearest; the filter "trilinear", which ``anisotropy`` above 1 needs, binds the texture with
    # its mip chain): every frame starts from cleared
    # buffers (one model per frame, as "fused") and the model's texture is mapped per pixel before the
    # illumination; with on_device="fused" the texture pass carries the light and the raster kernel does not shade.
    _Option("texture_pass", None, None),
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
    _Option("supersample", "resolve", "that keeps its planes on the device (AdvancedPixelBufferFiller, "
            "EdgeOnlyPixelBufferFiller): this one", clears=False),
    # shadow=None (default): no light is occluded.  A dict of ``filler`` (a second AdvancedPixelBufferFiller, the
    # light's: its frame is the shadow map), ``R`` and ``t`` (the light's frame, ``shadow.look_at``) and, optionally,
    # ``bias`` / ``pcf`` / ``ambient`` / ``use_winner`` (AdvancedPixelBufferFiller.shadow_pass's arguments): every
    # frame starts from cleared buffers (one model per frame, as "fused"), the model is drawn a second time from the
    # light, and the shadow pass runs on the camera's frame after any texture pass and before the illumination and
    # the resolve (with on_device="fused" the raster kernel or the texture pass has shaded already: the factors of
    # light and shadow commute up to rounding, the pass multiplies what it finds).
    _Option("shadow", "shadow_pass", "with a shadow pass (AdvancedPixelBufferFiller): this one",
            required=("filler", "R", "t"), missing="needs the keys 'filler', 'R' and 't': {missing} missing"),
    # ambient_occlusion=None (default): creases are lit like open surfaces.  A dict of AdvancedPixelBufferFiller.ao_pass's
    # arguments ({} = its defaults): every frame starts from cleared buffers (one model per frame, as "fused") and the
    # pass runs on the camera's frame after any texture pass and BEFORE the Phong pass, the shadow pass, the
    # illumination and the resolve: it scales the surface colour, so Phong's additive highlight is not dimmed.  With
    # on_device="fused" it multiplies what the raster kernel or the texture pass stored; with ``supersample=s`` it
    # runs on the supersampled frame, and ``radius_px`` counts that frame's pixels.
    _Option("ambient_occlusion", "ao_pass", "with an ambient-occlusion pass " + _PASS),
    # wireframe=None (default): no lines.  A dict of AdvancedPixelBufferFiller.wire_pass's arguments ({} = its defaults:
    # every edge, one pixel wide, white) and, optionally, ``feature_angle``: the edge mask is then
    # ``wireframe.feature_edges(the model's triangles, feature_angle)``, computed once per model.  Every frame starts
    # from cleared buffers (one model per frame, as "fused").  The lines are an overlay and are NOT lit: the pass
    # runs after everything that shades — the illumination in whichever form, the shadow pass under a
    # PhongIllumination — and before the resolve.  With ``supersample=s`` it runs on the supersampled frame, ``width``
    # counts that frame's pixels, and the light cannot ride in the resolve (it would shade the lines): the
    # illumination's device form runs over the supersampled frame, then the wire pass, then the plain resolve.
    # Its keys ``contours``, ``hidden`` and ``vector``: ``Renderer._check_wireframe``.
    _Option("wireframe", "wire_pass", "with a wireframe pass " + _PASS),
    # antialias=None (default): every pixel is its one sample.  A dict: geometric edge anti-aliasing
    # (``AdvancedPixelBufferFiller.edge_aa``) of the finished frame — {} smooths every edge, ``edges`` is an explicit
    # mask, and ``feature_angle`` / ``contours`` / ``borders`` pick the edges as ``wireframe`` picks them (the mask
    # and the partner table once per model, the contours of the view every frame).  Every frame starts from cleared
    # buffers (one model per frame, as "fused").  The pass runs LAST, after everything that shades and after the wire
    # pass, reads the filler's planes and writes a tensor of its own, which ``render`` returns: the tensor for
    # on_device=True / "fused", a fresh numpy copy for None / False (as under ``supersample``, with which it does
    # not combine).
    _Option("antialias", "edge_aa", "with an edge anti-aliasing pass " + _PASS, ("edges", "feature_angle", "contours", "borders"),
            excludes=("supersample",), clash="together with supersample=...: the pass smooths the frame's own pixels and "
            "does not combine with the resolve; use one of the two"),
    # depth_of_field=None (default): a pinhole image, sharp at every depth.  A dict of
    # ``AdvancedPixelBufferFiller.depth_of_field``'s arguments (``focus``, which it needs, and ``aperture`` / ``band`` /
    # ``max_radius``): a gather blur of the finished frame by every pixel's circle of confusion.  Every frame starts
    # from cleared buffers (one model per frame, as "fused").  The pass runs LAST, after everything that shades and
    # after the wire pass, reads the filler's planes and writes a tensor of its own, which ``render`` returns: the
    # tensor for on_device=True / "fused", a fresh numpy copy otherwise.  It combines neither with ``antialias`` (each
    # of the two reads the filler's colour plane and returns a plane of its own: the second would not see the first)
    # nor with ``supersample`` (the radii would count the supersampled frame's pixels, and the resolve reads the
    # filler's plane, not the pass's).
    _Option("depth_of_field", "depth_of_field", "with a depth-of-field pass " + _PASS, ("focus", "aperture", "band", "max_radius"),
            ("focus",), "needs 'focus', the view depth that stays sharp", ("antialias", "supersample"),
            "together with antialias=... or supersample=...: " + _OWN_PLANE + "blurred one; use one of them"),
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
    _Option("motion_blur", "motion_blur", "with a motion-blur pass " + _PASS, ("exposure", "max_radius", "taps", "soft"),
            excludes=("antialias", "depth_of_field", "supersample", "transparency"),
            clash="together with antialias=..., depth_of_field=..., supersample=... or transparency=...: " + _OWN_PLANE +
            "blurred one; use one of them"),
    # temporal_aa=None (default): every frame stands alone.  A dict of ``blend`` (default 0.1), ``jitter`` (an int from 0 to
    # 64, default 8: the length of the cycle of sub-pixel offsets, ``temporal.jitter_offsets``; 0 draws every frame
    # without an offset), ``dilate`` and ``clamp`` (``AdvancedPixelBufferFiller.temporal_resolve``'s arguments): temporal
    # anti-aliasing.  Frame n since the first ``render`` (or ``reset_motion()``, or a change of the triangle count) is
    # drawn from a stand-in for the model whose vertices are sheared by offset ``n mod jitter`` (``temporal.view_shear``,
    # ``sheared``: the image moves by that fraction of a pixel; texture, normal-map, shadow and edge helpers keep
    # receiving the caller's model), and the finished frame is blended into the image returned for the frame before,
    # reprojected along the motion vectors against the pose of the call before (a device COPY of every frame's
    # unjittered vertices is kept, as under ``motion_blur``; it is sheared by THIS frame's offset, so that the jitter
    # cancels in the velocity) with ``blend = max(blend, 1 / (n + 1))``: a still model averages its frames evenly until
    # the floor is reached.  Frame 0 is the jittered frame, copied.  Every frame starts from cleared buffers (one model
    # per frame, as "fused").  The pass runs LAST, after everything that shades and after the wire pass, reads the
    # filler's planes and writes a tensor of its own, which ``render`` returns (``bloom`` reads it) AND keeps as the next
    # history: clone it before editing it.  The tensor for on_device=True / "fused", a fresh numpy copy otherwise.  It
    # combines with none of ``antialias``, ``depth_of_field``, ``motion_blur``, ``supersample`` and ``transparency``:
    # each of them reads the filler's own colour plane and would not see the resolved one.
    _Option("temporal_aa", "temporal_resolve", "with a temporal resolve pass " + _PASS, ("blend", "jitter", "dilate", "clamp"),
            excludes=("antialias", "depth_of_field", "motion_blur", "supersample", "transparency"),
            clash="together with antialias=..., depth_of_field=..., motion_blur=..., supersample=... or transparency=...: " +
            _OWN_PLANE + "resolved one; use one of them"),
    # normal_map=None (default): the light sees the interpolated vertex normals.  A dict of
    # AdvancedPixelBufferFiller.bind_normal_map's arguments but the uv (``normal_map`` or ``height``, ``scale``, ``wrap``,
    # ``mipmaps``) and of normal_map_pass's (``strength``, ``perspective``, ``filter``; "trilinear" binds the map with
    # its mip chain): the map is bound at construction, once, and the model's texture coordinates once per model.  Every
    # frame starts from cleared buffers (one model per frame, as "fused") and the pass runs FIRST, directly after the draw:
    # it perturbs the normal plane, which the ambient occlusion, the fused light of the texture pass, the Phong
    # pass, the illumination and the resolve read afterwards.  With ``supersample=s`` it runs on the supersampled
    # frame.  on_device="fused" needs a ``texture_pass`` (which then carries the light): without one the raster
    # kernel has shaded from the unperturbed normals before any pass can run.
    _Option("normal_map", "normal_map_pass", "with a normal-map pass " + _PASS,
            ("normal_map", "height", "scale", "wrap", "mipmaps", "strength", "perspective", "filter")),
    # environment=None (default): nothing is mirrored and the background keeps the cleared colour.  A dict of ``faces``
    # (the cube map, uint8 [6, S, S, 3]: ``environment.cube_from_equirect`` / ``gradient_sky``) and, optionally,
    # ``mipmaps`` (AdvancedPixelBufferFiller.bind_environment's arguments) and ``reflectivity`` / ``f0`` / ``tint`` /
    # ``level`` / ``orientation`` / ``background`` (environment_pass's; a ``level`` above 0 binds the cube with its mip
    # chain): the cube is bound at construction, once.  Every frame starts from cleared buffers (one model per frame, as
    # "fused") and the pass runs AFTER the light in whichever form — the illumination's device or host form, the fused
    # light of the raster kernel or the texture pass, the Phong pass and its shadow pass — and immediately BEFORE the wire
    # pass, so that the lines and ``antialias`` come after it and silhouettes blend against the sky.  (The sky cannot
    # come before the light: the illumination multiplies the background by the factor of a zero normal.)  With
    # ``supersample=s`` it runs on the supersampled frame and the light cannot ride in the resolve (it would shade
    # the mirror image and the sky): as under ``wireframe``, the light runs as a pass of its own, then the
    # environment, then the wire pass, then the plain resolve.
    _Option("environment", "environment_pass", "with an environment pass " + _PASS,
            ("faces", "mipmaps", "reflectivity", "f0", "tint", "level", "orientation", "background")),
    # transparency=None (default): every pixel shows its nearest surface and nothing behind it.  A dict of
    # ``AdvancedPixelBufferFiller.transparency_pass``'s arguments (``alpha``, which it needs, and ``layers`` /
    # ``background`` / ``front``): the frame's depth layers peeled and blended front to back.  Every frame starts from
    # cleared buffers (one model per frame, as "fused").  The pass runs LAST, after everything that shades and after the
    # wire pass, reads the filler's planes and writes a tensor of its own, which ``render`` returns: the tensor for
    # on_device=True / "fused", a fresh numpy copy otherwise.  The layers behind the first are lit by the
    # ``light_direction`` of a GuroIllumination (or the key of that name); a PhongIllumination is refused, since they would be lit by another
    # model than the first.  It combines with none of ``antialias``, ``depth_of_field`` and ``supersample``.
    # (Checked after the illumination: its record and bloom's follow the Phong refusals.)
    _Option("transparency", "transparency_pass", "with a transparency pass " + _PASS,
            ("alpha", "layers", "light_direction", "background", "front"),
            ("alpha",), "needs 'alpha', a number or one value per triangle", ("antialias", "depth_of_field", "supersample"),
            "together with antialias=..., depth_of_field=... or supersample=...: " + _OWN_PLANE + "blended one; use one of them"),
    # bloom=None (default): what is brighter than 255 stays as the frame holds it.  A dict of the filler's ``bloom``
    # arguments but ``source`` ({} = its defaults: a glow of radius 8 around what exceeds 255): bloom and tone mapping
    # of the finished image.  It runs after EVERYTHING else and reads a source: the tensor of ``transparency``,
    # ``depth_of_field``, ``antialias`` or ``supersample``, whichever ran, or else the filler's colour plane — so it
    # combines with each of the four, and alone it changes nothing about how the frame is drawn.  ``render`` returns
    # the pass's own tensor for on_device=True / "fused", a fresh numpy copy otherwise.
    _Option("bloom", "bloom", "that keeps its planes on the device (AdvancedPixelBufferFiller, EdgeOnlyPixelBufferFiller): "
            "{filler}", _bloom_keys, clears=False),
)


class Renderer:
    """``render(model)`` draws one frame with the filler and returns its image.  The options are declared in ``_OPTIONS``
    above, each with its comment; a frame runs in this order (``_frame``): the draw, the normal map, the texture pass,
    the ambient occlusion, the shadow pass, the light, the environment, the wire pass (with its hidden lines and
    vectors), the resolve; under a PhongIllumination the shadow pass follows the light.  ``render`` then runs the one
    pass that reads the finished frame (``transparency``, ``depth_of_field``, ``motion_blur``, ``temporal_aa`` or
    ``antialias``) and
    ``bloom`` after everything else."""

    def __init__(self, pixel_buffer_filler, illumination, triangle_iterator_type=None,
                 image_height=512, image_width=512, use_tqdm=True, on_device=None, texture_pass=None,
                 shadow=None, ambient_occlusion=None, antialias=None, temporal_aa=None, depth_of_field=None, motion_blur=None,
                 normal_map=None, environment=None, bloom=None, transparency=None, wireframe=None, supersample=None):
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
        self._textured = None          # weak reference to the model whose texture the filler holds
        self._bumped = None            # weak reference to the model whose uv the normal map is bound with
        self._wired = None             # (weak reference to the model, its feature-edge mask, its partner table, the angle)
        self._smoothed = None          # as _wired, for the edges of ``antialias``
        self._paired = None            # (weak reference to the model, its partner table) where the contours keep none
        self._previous_pose = None     # the device copy of the (unjittered) vertices the last frame was drawn from
        self._history = None           # under temporal_aa: the tensor the last ``render`` resolved, the next history
        self._frame_number = 0         # under temporal_aa: n, the frames since the history began
        self.line_drawing = None       # the last frame's LineDrawing under wireframe={"vector": ...}
        # A PhongIllumination is a deferred pass of the filler over its winner plane (``phong_pass``): every frame
        # starts from cleared buffers (one model per frame, as "fused"); the draw, then the texture pass (unlit) if
        # asked for, then the Phong pass, then the shadow pass — AFTER the light here, since the specular term is
        # additive and a factor applied before it would leave highlights inside shadows: the shadow's ``ambient`` is
        # the floor of everything — then the plain resolve.  None returns the numpy colour view (with supersample a
        # fresh numpy copy), True the tensor.
        from .illumination.phong_illumination import PhongIllumination
        self._phong = isinstance(illumination, PhongIllumination)
        given = dict(texture_pass=texture_pass, shadow=shadow, ambient_occlusion=ambient_occlusion, antialias=antialias,
                     depth_of_field=depth_of_field, motion_blur=motion_blur, temporal_aa=temporal_aa, normal_map=normal_map,
                     environment=environment,
                     bloom=bloom, transparency=transparency, wireframe=wireframe, supersample=supersample)
        # what is one option's own: checked between the method and the keys, and how its dict is kept
        own_checks = {"wireframe": self._check_wireframe, "antialias": lambda v: self._check_contours("antialias", v),
                      "normal_map": lambda v: self._check_fused_normal_map(texture_pass),
                      "transparency": self._check_transparency, "temporal_aa": self._check_temporal}
        keep = {"normal_map": self._bind_normal_map, "environment": self._bind_environment, "supersample": lambda v: v}
        for o in _OPTIONS:
            if o.name == "transparency":
                self._check_phong()        # here, as ever: of two refusals in one call the first in this order is reported
            value = given[o.name]
            setattr(self, o.name, None)
            if value is None:
                continue
            self._check_filler(o, given)
            own_checks.get(o.name, lambda v: None)(value)
            self._check_keys(o, value)
            setattr(self, o.name, keep.get(o.name, dict)(value))
        # one model per frame: any pass but the resolve and bloom, and a Phong pass, need a frame that started cleared
        self._cleared = self._phong or any(o.clears and getattr(self, o.name) is not None for o in _OPTIONS)

    def _check_filler(self, o, given):
        """The two checks of the option `o` against the others and against the filler."""
        filler = self.pixel_buffer_filler
        if any(given[n] is not None for n in o.excludes):
            raise ValueError(f"Renderer({o.name}=...) {o.clash}")
        if o.method is not None and not hasattr(filler, o.method):
            raise ValueError(f"Renderer({o.name}=...) needs a filler {o.needs.format(filler=type(filler).__name__)} "
                             f"has no {o.method}()")

    @staticmethod
    def _check_keys(o, value):
        """The two checks of the keys of the option `o`'s dict `value`."""
        known = o.known() if callable(o.known) else o.known
        unknown = sorted(set(value) - set(known)) if known is not None else None
        if unknown:
            raise ValueError(f"Renderer({o.name}=...) takes the keys " + ", ".join(repr(k) for k in known[:-1]) +
                             f" and {known[-1]!r}: {unknown} unknown")
        missing = [k for k in o.required if k not in value]
        if missing:
            raise ValueError(f"Renderer({o.name}=...) " + o.missing.format(missing=missing))

    def _check_contours(self, name, options):
        # ``contours`` (True): the edge mask is rebuilt for every frame's view on the device
        # (``AdvancedPixelBufferFiller.contour_edges``) from the model's partner table (``wireframe.edge_partners``,
        # once per model, on the device for a device model): the contour edges, over the ``feature_angle`` mask or
        # an explicit ``edges`` if there is one, and with ``borders`` (default True) the rim of an open mesh.
        if options.get("contours") and not hasattr(self.pixel_buffer_filler, "contour_edges"):
            raise ValueError(f"Renderer({name}={{'contours': True}}) needs a filler that classifies contour edges "
                             f"(AdvancedPixelBufferFiller): {type(self.pixel_buffer_filler).__name__} has no contour_edges()")

    def _check_wireframe(self, wireframe):
        self._check_contours("wireframe", wireframe)
        # ``hidden`` (True, or a dict of AdvancedPixelBufferFiller.hidden_line_pass's arguments): the edges BEHIND the
        # surface, dashed, right after the wire pass and with the same mask of the view, so that the contours, creases
        # and borders of the far side are drawn; with ``supersample=s`` on the supersampled frame, whose pixels
        # ``dash`` counts.
        # ``vector`` (True, or a dict of AdvancedPixelBufferFiller.line_runs' arguments): after the wire pass and the
        # hidden pass of a frame the same view's drawing is also taken as vector segments, with the view's mask reduced
        # to one half-edge per edge (``wireframe.half_edges_once``) and the model's partner table (the contours' own, or
        # made once per model), and kept as ``renderer.line_drawing`` (``wireframe.write_svg`` writes it).  With
        # ``supersample=s`` its coordinates are the supersampled frame's.
        who = type(self.pixel_buffer_filler).__name__
        for key, method, needs, takes in (
                ("hidden", "hidden_line_pass", "with a hidden-line pass", "hidden_line_pass's"),
                ("vector", "line_runs", "that returns the drawing as vectors", "line_runs'")):
            value = wireframe.get(key)
            if value is not None and value is not False:
                if not hasattr(self.pixel_buffer_filler, method):
                    raise ValueError(f"Renderer(wireframe={{'{key}': ...}}) needs a filler {needs} "
                                     f"(AdvancedPixelBufferFiller): {who} has no {method}()")
                if value is not True and not isinstance(value, dict):
                    raise ValueError(f"Renderer(wireframe={{'{key}': ...}}) takes True or a dict of {takes} "
                                     f"arguments, got {value!r}")

    def _check_fused_normal_map(self, texture_pass):
        if self.on_device == "fused" and texture_pass is None:
            raise ValueError("Renderer(normal_map=..., on_device='fused') without a texture_pass: the raster kernel "
                             "shades from the unperturbed normals before any pass can run; add a texture_pass, which "
                             "carries the light, or use another on_device")

    def _bind_normal_map(self, normal_map):
        """Binds the map with the keys that are ``bind_normal_map``'s -> the keys that are the pass's."""
        opts = dict(normal_map)
        kept = {k: opts.pop(k) for k in ("strength", "perspective", "filter") if k in opts}
        if kept.get("filter") == "trilinear":
            opts.setdefault("mipmaps", True)
        self.pixel_buffer_filler.bind_normal_map(opts.pop("normal_map", None), **opts)
        if self.pixel_buffer_filler.get_normal_map() is None:
            raise ValueError("Renderer(normal_map=...) needs 'normal_map' or 'height'")
        return kept

    def _bind_environment(self, environment):
        """Binds the cube with the keys that are ``bind_environment``'s -> the keys that are the pass's."""
        opts = dict(environment)
        if opts.get("faces") is None:
            raise ValueError("Renderer(environment=...) needs 'faces'")
        level = opts.get("level", 0.0)
        if not isinstance(level, bool) and isinstance(level, (int, float, np.integer, np.floating)) and level > 0:
            opts.setdefault("mipmaps", True)
        self.pixel_buffer_filler.bind_environment(opts.pop("faces"), mipmaps=bool(opts.pop("mipmaps", False)))
        return opts

    def _check_phong(self):
        if self._phong:
            if self.on_device is False or self.on_device == "fused":
                raise ValueError(f"Renderer(on_device={self.on_device!r}) with a PhongIllumination: the model needs the winner "
                                 "plane and the triangles, so it has no host form on two planes and is not fused into "
                                 "the raster kernel; use on_device=None or True")
            if not hasattr(self.pixel_buffer_filler, "phong_pass"):
                raise ValueError("Renderer with a PhongIllumination needs a filler with a Phong pass "
                                 f"(AdvancedPixelBufferFiller): {type(self.pixel_buffer_filler).__name__} has no phong_pass()")

    def _check_transparency(self, transparency):
        if self._phong:
            raise ValueError("Renderer(transparency=...) with a PhongIllumination: the layers behind the first are shaded "
                             "with the Guro light or none and would be lit by another model than the first; use a "
                             "GuroIllumination")

    @staticmethod
    def _check_temporal(temporal_aa):
        jitter = temporal_aa.get("jitter", 8)
        if isinstance(jitter, bool) or not isinstance(jitter, (int, np.integer)) or not 0 <= jitter <= 64:
            raise ValueError(f"Renderer(temporal_aa=...): jitter must be an int from 0 to 64, got {jitter!r}")
        blend = temporal_aa.get("blend", 0.1)
        if isinstance(blend, bool) or not isinstance(blend, (int, float, np.integer, np.floating)) or not 0 < float(blend) <= 1:
            raise ValueError(f"Renderer(temporal_aa=...): blend must be a number above 0 and at most 1, got {blend!r}")

    def _frame(self, model, drawn=None):
        """One frame after the model fit, in the order the class documents -> (the image: the resolve's tensor, the
        colour tensor or the colour view; whether a resolve's tensor is handed out as it is, not as a numpy copy).
        `drawn`: the stand-in the filler draws in the model's place (``temporal_aa``); the helpers get the model."""
        filler, shading, s = self.pixel_buffer_filler, self.illumination, self.supersample
        drawn = model if drawn is None else drawn
        # where the light comes from: the raster kernel, the texture pass, the resolve, the illumination's device form,
        # its host form ("host" also where a device form is tried first), or the Phong pass
        device_form = None
        if self._phong:
            source, device_form = "phong", shading.draw_illumination_device
        elif self.on_device == "fused" and getattr(shading, "fuse_into", None):
            source = "raster" if self.texture_pass is None else "texture"
        else:
            source = "host"
            device_form = getattr(shading, "draw_illumination_device", None)
            if self.on_device is False or (self.on_device is None and not _device_form_is_the_same_shading(shading)):
                # (a subclass that overrides draw_illumination alone — the reference's only hook (renderer.py:47-49) —
                # gets ITS shading, on the host views, not the parent's device form)
                device_form = None
            elif s is None and not hasattr(filler, "get_color_tensor"):
                device_form = None
            elif s is not None and getattr(shading, "light_direction", None) is None:
                device_form = None
            if device_form is not None and s is not None and self.wireframe is None and self.environment is None:
                # the resolve carries the light: the supersampled colour plane is read once and stays unshaded.  (Not
                # with lines, a mirror image or a sky, which are not lit: the light then runs as a pass of its own.)
                source = "resolve"
        fused = source in ("raster", "texture")
        # the draw
        if source == "raster":
            shading.fuse_into(filler)
        if self.texture_pass is not None:
            self._bind_texture(model)
        if self._cleared:
            # (the views handed out so far are refreshed by the next getter call, after the passes; the raster kernel
            # shades only for the "fused" caller without a texture pass, whose colours would replace what it stores)
            if source != "raster":
                filler.set_fused_illumination(None)
            filler.render_model(drawn, clear=True, refresh_views=False)
        elif source == "raster":
            filler.render_model(drawn, clear=True)
        elif device_form is not None:
            filler.render_model(drawn, refresh_views=False)      # (the getter below refreshes the views, after the shading)
        else:
            filler.render_model(drawn)     # without ``clear``: renders composite, as in the reference
        # the passes before the light
        self._bump(model)                  # before the texture pass, whose fused light reads the normal plane
        if self.texture_pass is not None:
            filler.texture_pass(light_direction=shading.light_direction if source == "texture" else None, **self.texture_pass)
        if self.ambient_occlusion is not None:
            filler.ao_pass(**self.ambient_occlusion)
        if self.shadow is not None and not self._phong:
            self._cast_shadows(model)
        # the light
        lit_on_device = device_form is not None and source != "resolve" and bool(device_form(filler) or self._phong)
        if source == "host" and not lit_on_device:
            shading.draw_illumination(filler.get_color_buffer(), filler.get_normals_buffer())
        if self.shadow is not None and self._phong:
            self._cast_shadows(model)
        # what is not lit (after a host illumination it carries the host edits to the device; the view shows the lines)
        if self.environment is not None:
            filler.environment_pass(**self.environment)
        if self.wireframe is not None:
            self._draw_wire(model)
        # the result
        if s is not None:
            image = filler.resolve(s, light_direction=shading.light_direction) if source == "resolve" else filler.resolve(s)
            return image, fused or (self.on_device is True and device_form is not None)
        if fused or (self.on_device is True and lit_on_device):
            return filler.get_color_tensor(), True
        return filler.get_color_buffer(), True

    def _bind_texture(self, model):
        """The model's texture and texture coordinates to the filler, once per model, not per frame."""
        if self._textured is None or self._textured() is not model:
            getters = [getattr(model, n, None) for n in ("get_texture_coords_by_triangles", "get_texture")]
            uv, tex = [g() if g is not None else None for g in getters]
            if uv is None or tex is None:
                raise ValueError("Renderer(texture_pass=...) needs a textured model: this one has no texture "
                                 "coordinates or no texture image")
            if self.texture_pass.get("filter") == "trilinear":
                self.pixel_buffer_filler.bind_texture(uv, tex, mipmaps=True)
            else:
                self.pixel_buffer_filler.bind_texture(uv, tex)
            self._textured = weakref.ref(model)

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
        """The wire pass over the frame as it stands (host edits included), then its hidden lines and its vectors."""
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

    def _once(self, model, slot, make):
        """The once-per-model cache `slot`, a tuple that starts with a weak reference to its model: as it stands if it
        is `model`'s, else ``(the reference, *make(carry))`` kept there, `carry` moving an array to the filler's device."""
        cache = getattr(self, slot)
        if cache is None or cache[0]() is not model:
            device = getattr(self.pixel_buffer_filler, "device", None)

            def carry(array):              # (a device model's table is made on the device)
                if device is not None and not hasattr(array, "data_ptr"):
                    import torch
                    array = torch.from_numpy(array).to(device)
                return array
            cache = (weakref.ref(model), *make(carry))
            setattr(self, slot, cache)
        return cache

    def _partners(self, model):
        """The model's partner table: the one the contours of ``wireframe`` hold, or one made once per model."""
        if self._wired is not None and self._wired[0]() is model and self._wired[2] is not None:
            return self._wired[2]
        from .wireframe import edge_partners
        return self._once(model, "_paired", lambda carry: (carry(edge_partners(model._vertices_by_triangles)),))[1]

    def _view_edges(self, model, options, slot):
        """`options` (``wireframe``'s or ``antialias``'s) with ``feature_angle`` / ``contours`` / ``borders`` turned into
        the ``edges`` of this frame's view.  `slot` names the once-per-model cache, (weak reference to the model, mask,
        partner table, angle); what the other option's cache holds for the same model is taken from there."""
        opts = dict(options)
        angle = opts.pop("feature_angle", None)
        contours, borders = opts.pop("contours", False), opts.pop("borders", True)

        def make(carry):
            from .wireframe import edge_partners, feature_edges
            other = self._smoothed if slot == "_wired" else self._wired
            if other is None or other[0]() is not model:
                other = (None, None, None, None)
            tri = model._vertices_by_triangles
            mask = partners = None
            if angle is not None:
                mask = other[1] if other[1] is not None and other[3] == angle else \
                    carry(feature_edges(tri.cpu().numpy() if hasattr(tri, "cpu") else tri, angle))
            if contours:
                partners = other[2] if other[2] is not None else carry(edge_partners(tri))
            return mask, partners, angle
        if angle is not None or contours:
            cache = self._once(model, slot, make)
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
        filler = self.pixel_buffer_filler
        shear = self._jitter(model) if self.temporal_aa is not None else None
        if shear is None:
            image, as_it_is = self._frame(model)
        else:
            from .temporal import JitteredModel
            image, as_it_is = self._frame(model, JitteredModel(model, *shear))
        # the frame as ever, then the one pass that reads the finished frame, last of all: its own tensor is the image
        last = None
        if self.transparency is not None:
            opts = dict(self.transparency)
            opts.setdefault("light_direction", getattr(self.illumination, "light_direction", None))
            last = filler.transparency_pass(**opts)
        elif self.depth_of_field is not None:
            last = filler.depth_of_field(**self.depth_of_field)
        elif self.motion_blur is not None:
            last = self._shutter(model)
        elif self.temporal_aa is not None:
            last = self._accumulate(model, shear)
        elif self.antialias is not None:
            last = filler.edge_aa(**self._view_edges(model, self.antialias, "_smoothed"))
        if self.bloom is not None:
            # after everything else: over the tensor of the pass that ran last or of the resolve, or over the filler's
            # own colour plane, host edits included, which bloom completes itself (``source=None``)
            last = filler.bloom(source=image if last is None and self.supersample is not None else last, **self.bloom)
        if last is not None:
            image, as_it_is = last, self.on_device is True or self.on_device == "fused"
        return image if as_it_is else image.cpu().numpy()

    def _pose_copy(self, model):
        """A device copy of the vertex array of `model` as it is now (a DeviceModel is transformed in place)."""
        import torch
        v = model._vertices_by_triangles
        device = getattr(self.pixel_buffer_filler, "device", None)
        if isinstance(v, torch.Tensor):
            return v.detach().to(device=v.device if device is None else device, copy=True)
        current = torch.from_numpy(np.array(v, copy=True))
        return current if device is None else current.to(device)

    def _jitter(self, model):
        """(kx, ky), the view shear of this frame under ``temporal_aa``, or None where it is drawn without an offset.  A
        first frame, and one whose triangle count is not the kept pose's, is frame 0."""
        previous = self._previous_pose
        if previous is None or self._history is None or previous.shape[0] != len(model._vertices_by_triangles):
            self._frame_number = 0
        J = int(self.temporal_aa.get("jitter", 8))
        if J == 0:
            return None
        from .temporal import jitter_offsets, view_shear
        filler = self.pixel_buffer_filler
        jx, jy = jitter_offsets(J)[self._frame_number % J]
        return view_shear(filler._P, filler.h, filler.w, jx, jy)

    def _accumulate(self, model, shear):
        """The temporal resolve over the frame just drawn, against the image and the pose of the call before; keeps this
        call's unjittered pose and the resolved image."""
        opts = dict(self.temporal_aa)
        opts.pop("jitter", None)
        n, floor = self._frame_number, float(opts.pop("blend", 0.1))
        current = self._pose_copy(model)
        if n == 0:
            image = self.pixel_buffer_filler.temporal_resolve(None)         # the frame, copied
        else:
            previous = self._previous_pose
            if shear is not None:
                from .temporal import sheared
                previous = sheared(previous, *shear)
            image = self.pixel_buffer_filler.temporal_resolve(self._history, previous_vertices=previous,
                                                              blend=max(floor, 1.0 / (n + 1)), **opts)
        self._previous_pose, self._history, self._frame_number = current, image, n + 1
        return image

    def _shutter(self, model):
        """The motion-blur pass over the frame just drawn, against the pose of the call before; keeps this call's pose."""
        current = self._pose_copy(model)
        previous = self._previous_pose
        if previous is None or previous.shape[0] != current.shape[0]:
            previous = current         # a static pose: the frame, copied
        self._previous_pose = current
        return self.pixel_buffer_filler.motion_blur(previous, **self.motion_blur)

    def reset_motion(self):
        """Forget the previous pose: the next ``render`` under ``motion_blur`` returns its frame unblurred (a camera cut).
        Under ``temporal_aa`` the history is forgotten with it and the frames are counted from 0 again."""
        self._previous_pose = None
        self._history = None
        self._frame_number = 0

    def reset_buffers(self):
        pass   # a no-op in the reference too (renderer.py:51-52): renders composite
