"""The deferred passes of ``AdvancedPixelBufferFiller`` over the winner plane of its last frame: texture (nearest,
bilinear, trilinear, anisotropic), shadow, Phong, ambient occlusion and the wireframe overlay, and normal mapping (``normal_map_pass``: the one that writes the
normal plane the others read) and environment mapping (``environment_pass``: reflections and a skybox from a cube map), with the
texture, normal-map, environment and shadow-map bindings they read, the classification of a view's contour edges for the overlay (``contour_edges``: it reads no plane), the edges behind
the surface, dashed (``hidden_line_pass``: it walks the edges, not the winner plane's pixels, and keeps a key plane), the same
classification kept as vector segments (``line_runs``: it only reads the planes and returns a ``LineDrawing``) and geometric
edge anti-aliasing (``edge_aa``: it reads the planes and returns a plane of its own) and depth of field (``depth_of_field``:
a gather blur by the circle of confusion over the z plane, which returns a plane of its own as well), motion vectors and
motion blur (``motion_vectors`` and ``motion_blur``: where every pixel's surface point was in an earlier pose, and a gather
along that, two planes of their own), temporal anti-aliasing (``temporal_resolve``: the frame blended into a history
image that follows the surface, a plane of its own too) and transparency
(``peel_layers`` and ``transparency_pass``: the frame's depth layers peeled by depth key and blended front to back, a plane of its own again).  A mixin
beside ``_device_planes.DevicePlanes``: the filler supplies ``device, h, w, y0, y1, _lib, _P`` and its frame state (``_pipeline, _inputs, _order, _last_flags, _check_bins``).  What every pass has in common is here
once: whom it refuses (``_pass_target``), which frame it accepts (``_pass_frame``), and how it is launched
(``_run_pass``, whose leaf ``_launch_pass`` alone needs the GPU and the library).  A ``*_pass`` method holds its own argument checks and operands.  Also here, because the shadow
binding converts its vertices as the filler's upload does: the model arrays' way to float32."""
import ctypes as C
import operator

import numpy as np
import torch

from .. import _capi


def _host_f32(a):
    """numpy view of a float32 host array, with what the reference raises for None (``None.copy()``)
    and for another dtype (.pyx:94-96 binds ``float[:, :, :]``)."""
    if a is None:
        raise AttributeError("'NoneType' object has no attribute 'copy'")
    arr = np.asarray(a)
    if arr.dtype != np.float32:
        kind = "double" if arr.dtype == np.float64 else str(arr.dtype)
        raise ValueError(f"Buffer dtype mismatch, expected 'float' but got '{kind}'")
    return arr


def _check_host_f32(a, name):
    """numpy view of a [T, 3, 3] float32 host array (any strides), with the reference's errors."""
    arr = _host_f32(a)
    if arr.ndim != 3 or arr.shape[1] != 3 or arr.shape[2] != 3:
        raise ValueError(f"{name} must have shape [T, 3, 3], got {tuple(arr.shape)}")
    return arr


def _as_device_f32(a, name, device):
    """[T, 3, 3] float32 contiguous tensor on `device` from numpy / torch input."""
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.float32:
            raise ValueError(f"Buffer dtype mismatch, expected 'float' but got '{a.dtype}' ({name})")
        t = a.to(device=device).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(_host_f32(a))).to(device)
    if t.dim() != 3 or t.shape[1] != 3 or t.shape[2] != 3:
        raise ValueError(f"{name} must have shape [T, 3, 3], got {tuple(t.shape)}")
    return t


def _device_array(filler, a, dtype, shape_ok, what, part=slice(None)):
    """`a`, a numpy array or a tensor, as a contiguous tensor on the filler's device, which is looked at only after the
    check ("`what`, got <dtype> <shape>" unless its dtype is `dtype` and `shape_ok(its shape)`); `part` of it is moved."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != dtype or not shape_ok(tuple(t.shape)):
        raise ValueError(f"{what}, got {t.dtype} {tuple(t.shape)}")
    return t[part].to(filler.device).contiguous()


def _edge_mask(filler, edges, T):
    """None, or the uint8 [T] edge mask of ``wire_pass`` and ``edge_aa`` on the filler's device, from numpy or a tensor."""
    if edges is None:
        return None
    return _device_array(filler, edges, torch.uint8, lambda s: s == (T,),
                         f"edges must be uint8 [T] with T = {T}, the triangles of the last frame")


class LineDrawing:
    """What ``line_runs`` returns: ``runs`` int32 [N, 4] (segment, first step, last step, class) and ``ends`` float32
    [N, 4] (x0, y0, x1, y1) in the pixel coordinates of a frame ``height`` x ``width``, row k of both for run k."""
    HIDDEN, VISIBLE = 1, 2

    def __init__(self, runs, ends, height, width):
        self.runs, self.ends, self.height, self.width = runs, ends, int(height), int(width)

    def __len__(self):
        return int(self.runs.shape[0])

    def visible(self):
        """The ``ends`` rows of the visible runs, in order."""
        return self.ends[self.runs[:, 3] == self.VISIBLE]

    def hidden(self):
        """The ``ends`` rows of the hidden runs, in order."""
        return self.ends[self.runs[:, 3] == self.HIDDEN]


class DeferredPasses:
    _texture = None   # (uv [T, 3, 2] float32, image [th, tw, 3] uint8) device tensors: bind_texture
    _mip = None        # (chain, [(h_k, w_k)], [byte offsets]) of that image: bind_texture(mipmaps=True)
    _normal_map = None  # (uv [T, 3, 2] float32 or None, map [mh, mw, 3] uint8, its mip chain or None): bind_normal_map
    _environment = None  # (faces [6, S, S, 3] uint8, its mip chain over the faces stacked by rows or None): bind_environment
    _shadow = None     # (the light's filler, its vertices [T, 3, 3] float32 on the device): bind_shadow_map
    _hidden_key = None  # the zeroed int32 [h, w] key plane of hidden_line_pass, which every call leaves zero
    _peel_scratch = None  # (keys int64 [h, w], transmittance float32 [h, w], winners int32 [2, h, w], z float32 [2, h, w])

    # --------------------------------------------------- what every pass shares --
    def _pass_target(self, name):
        """Refuses the pass `name` on a filler whose planes rotate or that keeps no winner plane."""
        if self._pipeline:
            raise ValueError(f"{name} is not available on a swap chain (pipeline=True): per-slot passes are not implemented")
        if self.winner_buffer is None:
            raise ValueError(f"{name} needs the winner plane: construct the filler with track_winner=True")

    def _pass_frame(self, name, who=None):
        """(tri, T) of this filler's last frame, which must have started from cleared buffers.  `who` names the
        filler in the messages of a pass that reads two."""
        by, of, mixed = ("", "", "the winner plane of a composite mixes the triangle indices of several models") if who is None \
            else (f" by {who}", f" of {who}", "the planes of a composite mix several models")
        if self._inputs is None:
            raise ValueError(f"{name}: no frame has been rendered{by}")
        if not (self._last_flags & _capi.FUSED_CLEAR):
            raise ValueError(f"{name}: the last frame{of} did not start from cleared buffers (clear=True): {mixed}")
        tri = self._inputs[0]
        return tri, tri.shape[0]

    def _run_pass(self, entry, tri, T, operands, flags=0, more=(), z=False, light=None, reads_only=False, target=None):
        """Settle the frame and call the library's `entry` on torch's current stream:
        ``entry(winner, [z,] tri or NULL, T, pos_of, P, *operands, color, h, w, y0, y1, flags, *more, stream)``.
        Tensors among `operands` are passed by address, taken after the settle.  `light`: a second filler whose
        planes the pass reads, settled first.  `reads_only`: the pass writes none of the filler's planes, so the host
        views stay as fresh or as stale as they were.  `target`: the plane the pass writes in the colour plane's place."""
        self._push_host_edits()
        if light is not None:
            light._push_host_edits()
            light._check_bins()        # the map the pass reads is the light's final z
        self._check_bins()             # nothing pending from here on: no later redo can undo the pass
        pos_of = None if self._order is None else self._order[1]
        args = (self.winner_buffer,) + ((self.z_buffer,) if z else ()) + (tri if T else None, T, pos_of, self._P) + \
            tuple(operands) + (self.color_buffer if target is None else target, self.h, self.w, self.y0, self.y1, flags) + \
            tuple(more)
        self._launch_pass(entry, args)
        if not reads_only:
            self._host_fresh = False   # views handed out earlier show the pass's colours at the next getter call

    def _launch_pass(self, entry, args):
        """The leaf of ``_run_pass`` that needs the GPU and the library: `entry` on torch's current stream, the tensors
        among `args` by address."""
        with torch.cuda.device(self.device):
            _capi.check(getattr(self._lib, entry)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                                  self._stream()), entry)

    # ------------------------------------------------- bindings and the passes --
    def bind_texture(self, uv_by_triangles, texture, mipmaps=False):
        """Keep a texture resident for ``texture_pass``: `uv_by_triangles` float32 [T, 3, 2] (u, v per corner,
        in the caller's triangle order: ``Model.get_texture_coords_by_triangles()``) and `texture` uint8
        [th, tw, 3] (``Model.get_texture()``), numpy arrays or device tensors.  With `mipmaps` the texture's
        mip chain is built on the device as well (``crender_mip_build``, on torch's current stream), which
        ``texture_pass(filter="trilinear")`` needs.  ``bind_texture(None, None)`` drops both."""
        if uv_by_triangles is None and texture is None:
            self._texture = self._mip = None
            return
        if uv_by_triangles is None or texture is None:
            raise ValueError("bind_texture needs both the texture coordinates and the texture (or None, None)")
        uv = _device_array(self, uv_by_triangles, torch.float32, lambda s: len(s) == 3 and s[1:] == (3, 2),
                           "uv_by_triangles must be float32 [T, 3, 2]")
        tex = _device_array(self, texture, torch.uint8, lambda s: len(s) == 3 and s[2] >= 3 and s[0] >= 1 and s[1] >= 1,
                            "texture must be uint8 [th, tw, 3]", part=(..., slice(3)))
        self._mip = self._build_mip_chain(tex) if mipmaps else None
        self._texture = (uv, tex)

    def _build_mip_chain(self, tex):
        """(chain uint8 [total bytes], [(h_k, w_k)], [byte offset of level k]) of a device texture."""
        th, tw = int(tex.shape[0]), int(tex.shape[1])
        n = _capi.MIP_MAX_LEVELS
        levels, total = C.c_int32(0), C.c_uint64(0)
        hs, ws, offs = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_uint64 * n)()
        _capi.check(self._lib.crender_mip_layout(th, tw, C.byref(levels), hs, ws, offs, C.byref(total)),
                    "crender_mip_layout")
        chain = torch.empty(total.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.crender_mip_build(tex.data_ptr(), th, tw, chain.data_ptr(), self._stream()),
                        "crender_mip_build")
        L = levels.value
        return chain, [(hs[k], ws[k]) for k in range(L)], [offs[k] for k in range(L)]

    def mip_levels(self):
        """[(h_k, w_k)] of the bound texture's mip chain, or None without one."""
        return None if self._mip is None else list(self._mip[1])

    def get_mip_level(self, k):
        """Level `k` of the mip chain: a uint8 [h_k, w_k, 3] device tensor that views the chain."""
        if self._mip is None:
            raise ValueError("no mip chain is bound: bind_texture(..., mipmaps=True)")
        chain, levels, offsets = self._mip
        if not 0 <= k < len(levels):
            raise IndexError(f"the chain has levels 0 .. {len(levels) - 1}, got {k}")
        h, w = levels[k]
        return chain[offsets[k]:offsets[k] + 3 * h * w].view(h, w, 3)

    def texture_pass(self, perspective=False, filter="nearest", light_direction=None, anisotropy=1):
        """Per-pixel texture mapping of the LAST frame's colour plane (``crender_tex_shade``,
        include/crender_tex.h): every pixel a triangle won gets the bound texture's texel at its
        interpolated (u, v) — affine like the reference's attributes, or perspective-correct; the nearest
        texel or four of them — instead of the blend of three vertex colours.  ``filter="trilinear"``
        (``crender_mip_shade``, include/crender_mip.h) picks a mip level per pixel from the screen-space
        derivatives of (u, v) and blends the bilinear samples of two levels; it needs the chain of
        ``bind_texture(..., mipmaps=True)``.  With `anisotropy` A from 2 to 16 on top of it
        (``crender_aniso_shade``, include/crender_aniso.h) the level comes from the shorter of a pixel's two
        texel-space steps, never more than A times shorter than the longer, and up to A trilinear samples
        span the longer one: a surface seen at a grazing angle keeps its detail across the short axis.  Rows of
        the filler's ``row_strip``, on torch's current stream.  With `light_direction` (the illumination object's own
        flipped, normalised vector, as ``set_fused_illumination`` takes it) the pass also shades every
        pixel of the rows: the same bits as the separate illumination pass afterwards, without its
        traffic.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin
        lists overflowed is rendered again, and the pass must land on the frame that stays."""
        if filter not in ("nearest", "bilinear", "trilinear"):
            raise ValueError(f"filter must be 'nearest', 'bilinear' or 'trilinear', got {filter!r}")
        if isinstance(anisotropy, bool) or not isinstance(anisotropy, int) or not 1 <= anisotropy <= _capi.ANISO_MAX:
            raise ValueError(f"anisotropy must be an int from 1 to {_capi.ANISO_MAX}, got {anisotropy!r}")
        if anisotropy > 1 and filter != "trilinear":
            raise ValueError(f"anisotropy={anisotropy} needs filter=\"trilinear\" (and its mip chain), got {filter!r}")
        self._pass_target("texture_pass")
        if self._texture is None:
            raise ValueError("texture_pass: no texture is bound (bind_texture)")
        if filter == "trilinear" and self._mip is None:
            raise ValueError("filter 'trilinear' needs a mip chain: bind_texture(..., mipmaps=True)")
        tri, T = self._pass_frame("texture_pass")
        uv, tex = self._texture
        if uv.shape[0] != T:
            raise ValueError(f"texture_pass: {uv.shape[0]} triangles of texture coordinates are bound, the last frame drew {T}")
        light = None if light_direction is None else (C.c_float * 3)(*[float(v) for v in light_direction])
        more = ()
        if filter == "trilinear":
            entry, image = "crender_mip_shade", self._mip[0]
            flags = _capi.MIP_PERSPECTIVE if perspective else 0
            if anisotropy > 1:
                entry, more = "crender_aniso_shade", (anisotropy,)
        else:
            entry, image = "crender_tex_shade", tex
            flags = (_capi.TEX_PERSPECTIVE if perspective else 0) | (_capi.TEX_BILINEAR if filter == "bilinear" else 0)
        self._run_pass(entry, tri, T, (uv if T else None, image, int(tex.shape[0]), int(tex.shape[1]),
                                       None if light is None else self.normals_buffer, light), flags, more)

    def bind_normal_map(self, normal_map=None, *, height=None, scale=1.0, wrap=False, uv_by_triangles=None, mipmaps=False):
        """Keep a tangent-space normal map resident for ``normal_map_pass``: `normal_map` uint8 [mh, mw, 3]
        (byte = 128 + 127 * component of a unit vector along u, along v and out of the surface; row 0 is the top of the
        image), or `height` uint8 [mh, mw], from which the map is made on the device (``crender_nmap_from_height``,
        include/crender_nmap.h, on torch's current stream): central differences times ``scale / 255``, the neighbours
        clamped to the edge or, with `wrap`, wrapped around.  Exactly one of the two, numpy arrays or device tensors; both
        None drops the binding.  `uv_by_triangles` float32 [T, 3, 2] (``bind_texture``'s) are the map's own coordinates;
        None means those of ``bind_texture`` at the time the pass runs.  With `mipmaps` the map's mip chain is built as
        a texture's is (the box average of the bytes), which ``normal_map_pass(filter="trilinear")`` needs."""
        if normal_map is None and height is None:
            self._normal_map = None
            return
        if normal_map is not None and height is not None:
            raise ValueError("bind_normal_map takes the normal map or the height map, not both")
        number = (int, float, np.integer, np.floating)
        if isinstance(scale, bool) or not isinstance(scale, number) or not np.isfinite(np.float32(scale)):
            raise ValueError(f"scale must be a finite number, got {scale!r}")
        side = lambda s: 1 <= s[0] <= 65535 and 1 <= s[1] <= 65535
        uv = None
        if uv_by_triangles is not None:
            uv = _device_array(self, uv_by_triangles, torch.float32, lambda s: len(s) == 3 and s[1:] == (3, 2),
                               "uv_by_triangles must be float32 [T, 3, 2]")
        if height is None:
            nmap = _device_array(self, normal_map, torch.uint8, lambda s: len(s) == 3 and s[2] >= 3 and side(s),
                                 "normal_map must be uint8 [mh, mw, 3] with sides from 1 to 65535", part=(..., slice(3)))
        else:
            hm = _device_array(self, height, torch.uint8, lambda s: len(s) == 2 and side(s),
                               "height must be uint8 [mh, mw] with sides from 1 to 65535")
            mh, mw = int(hm.shape[0]), int(hm.shape[1])
            nmap = torch.empty((mh, mw, 3), dtype=torch.uint8, device=self.device)
            self._launch_pass("crender_nmap_from_height", (hm, mh, mw, float(scale), _capi.NMAP_WRAP if wrap else 0, nmap))
        self._normal_map = (uv, nmap, self._build_mip_chain(nmap) if mipmaps else None)

    def bind_normal_map_uv(self, uv_by_triangles):
        """Replace the coordinates of the bound normal map and keep the map: `uv_by_triangles` float32 [T, 3, 2], or None
        for those of ``bind_texture``.  (``Renderer(normal_map=...)`` binds the map once and the model's uv per model.)"""
        if self._normal_map is None:
            raise ValueError("bind_normal_map_uv: no normal map is bound (bind_normal_map)")
        uv = None
        if uv_by_triangles is not None:
            uv = _device_array(self, uv_by_triangles, torch.float32, lambda s: len(s) == 3 and s[1:] == (3, 2),
                               "uv_by_triangles must be float32 [T, 3, 2]")
        self._normal_map = (uv,) + self._normal_map[1:]

    def get_normal_map(self):
        """The bound normal map, a uint8 [mh, mw, 3] device tensor, or None without a binding."""
        return None if self._normal_map is None else self._normal_map[1]

    def normal_map_pass(self, strength=1.0, perspective=True, filter="bilinear"):
        """Normal (bump) mapping of the LAST frame's NORMAL plane (``crender_nmap_shade``, include/crender_nmap.h): every
        covered pixel samples the bound map at its interpolated (u, v) — the nearest texel, four of them, or
        (``"trilinear"``, which needs ``bind_normal_map(..., mipmaps=True)``) two levels of the map's mip chain picked
        from the screen-space derivatives of (u, v) —, decodes the tangent-space vector, scales its two tangent
        components by `strength`, and replaces its stored normal by that vector in the frame made of the normal itself
        and the winner's tangents (the directions of increasing u and v on the triangle, turned around the normal).  Run
        it right after the draw: the illumination, the fused light of ``texture_pass`` and ``resolve``, ``phong_pass`` and
        ``ao_pass(normals="plane")`` all read that plane and show the bumps.  A flat texel (128, 128, 255), ``strength=0``,
        degenerate uv and the background leave a pixel's bits alone; colour, z and winners are never written.  Rows of
        the filler's ``row_strip``, on torch's current stream.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin lists
        overflowed is rendered again, and the pass must land on the frame that stays."""
        if filter not in ("nearest", "bilinear", "trilinear"):
            raise ValueError(f"filter must be 'nearest', 'bilinear' or 'trilinear', got {filter!r}")
        if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) \
                or not np.isfinite(np.float32(strength)):
            raise ValueError(f"strength must be a finite number, got {strength!r}")
        self._pass_target("normal_map_pass")
        if self._normal_map is None:
            raise ValueError("normal_map_pass: no normal map is bound (bind_normal_map)")
        uv, nmap, chain = self._normal_map
        if filter == "trilinear" and chain is None:
            raise ValueError("filter 'trilinear' needs a mip chain: bind_normal_map(..., mipmaps=True)")
        if uv is None:
            if self._texture is None:
                raise ValueError("normal_map_pass: no texture coordinates are bound (bind_normal_map(..., uv_by_triangles=...) "
                                 "or bind_texture)")
            uv = self._texture[0]
        tri, T = self._pass_frame("normal_map_pass")
        if uv.shape[0] != T:
            raise ValueError(f"normal_map_pass: {uv.shape[0]} triangles of texture coordinates are bound, the last frame drew {T}")
        flags = (_capi.NMAP_PERSPECTIVE if perspective else 0) | (_capi.NMAP_BILINEAR if filter == "bilinear" else 0) | \
            (_capi.NMAP_CHAIN if filter == "trilinear" else 0)
        self._run_pass("crender_nmap_shade", tri, T,
                       (uv if T else None, chain[0] if filter == "trilinear" else nmap, int(nmap.shape[0]), int(nmap.shape[1]),
                        float(strength)), flags, target=self.normals_buffer)

    def bind_environment(self, faces, mipmaps=False):
        """Keep a cube map resident for ``environment_pass``: `faces` uint8 [6, S, S, 3] with S from 1 to 8192, a numpy
        array or a device tensor, the faces in the order +x, -x, +y, -y, +z, -z of the camera's frame (x grows with the
        column, y with the row, z goes into the screen; ``environment.cube_from_equirect`` and ``environment.gradient_sky``
        make one).  ``bind_environment(None)`` drops the binding.  With `mipmaps` S must be a power of two, and the chain
        is the texture's own (``crender_mip_build``, on torch's current stream) of the faces stacked by rows, a
        [6 S, S, 3] image: a 2 x 2 box never straddles two faces while the side is even, so of that chain the levels
        j = 0 .. log2 S are used, level j a [6 S / 2^j, S / 2^j, 3] image at the chain's byte offset of level j, in which
        face k starts ``k * 3 * (S / 2^j) ** 2`` bytes further on: six box-averaged faces of side S / 2^j.  (The chain's
        levels beyond log2 S average across faces and are never read.)"""
        if faces is None:
            self._environment = None
            return
        top = _capi.ENV_MAX_SIDE
        cube = _device_array(self, faces, torch.uint8,
                             lambda s: len(s) == 4 and s[0] == 6 and s[1] == s[2] and 1 <= s[1] <= top and s[3] >= 3,
                             f"faces must be uint8 [6, S, S, 3] with S from 1 to {top}", part=(..., slice(3)))
        S = int(cube.shape[1])
        chain = None
        if mipmaps:
            if S & (S - 1):
                raise ValueError(f"bind_environment(mipmaps=True) needs a side that is a power of two, got {S}")
            chain = self._build_mip_chain(cube.view(6 * S, S, 3))
        self._environment = (cube, chain)

    def get_environment(self):
        """The bound cube map, a uint8 [6, S, S, 3] device tensor, or None without a binding."""
        return None if self._environment is None else self._environment[0]

    def environment_levels(self):
        """The sides of the bound cube's levels: [S, S / 2, ..., 1] with a chain, [S] without; None without a binding."""
        if self._environment is None:
            return None
        cube, chain = self._environment
        S = int(cube.shape[1])
        return [S] if chain is None else [S >> j for j in range(S.bit_length())]

    def get_environment_level(self, j):
        """Level `j` of the bound cube: a uint8 [6, S / 2^j, S / 2^j, 3] device tensor that views the chain (level 0 of a
        cube without a chain is the cube)."""
        sides = self.environment_levels()
        if sides is None:
            raise ValueError("no environment is bound (bind_environment)")
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not 0 <= j < len(sides):
            raise IndexError(f"the environment has levels 0 .. {len(sides) - 1}, got {j!r}")
        cube, chain = self._environment
        if chain is None:
            return cube
        off, side = chain[2][j], sides[j]
        return chain[0][off:off + 18 * side * side].view(6, side, side, 3)

    def environment_pass(self, reflectivity=1.0, f0=0.04, tint=(1.0, 1.0, 1.0), level=0.0, orientation=None, background=None):
        """Environment mapping of the LAST frame's colour plane (``crender_env_shade``, include/crender_env.h) from the
        cube bound with ``bind_environment``.  Every covered pixel mirrors the direction from the eye to the surface
        point it shows (the perspective-correct blend of the winner's corners, as ``phong_pass`` takes it) at its stored
        normal, looks the mirrored direction up in the cube (the face of its largest component, four texels of it,
        nothing filtered across faces) and blends its colour c towards ``sample * tint`` by
        ``w = reflectivity * (f0 + (1 - f0) * (1 - cos) ** 5)``, cos between the normal and the way to the eye: `f0` is
        the share mirrored head-on (0.04 a glossy dielectric, 1 a mirror at every angle), and every surface mirrors at a
        grazing angle.  `level` is a position in the chain of ``bind_environment(..., mipmaps=True)``, 0 to its last
        level: the samples of the two levels around it are blended by its fraction, a blur (box averages, not a roughness
        model).  `orientation` is None or a 3 x 3 matrix that takes a direction of the camera's frame into the cube's.
        `background` — True, or a number, the gain — also gives every pixel of the rows that no triangle won the cube's
        colour along its own view ray (times the gain): a skybox; None or False leaves the background alone.  With
        ``reflectivity=0`` only the background is painted (and without one nothing is launched).  z, normals and winners
        are only read.  Rows of the filler's ``row_strip``, on torch's current stream.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin lists
        overflowed is rendered again, and the pass must land on the frame that stays."""
        number = (int, float, np.integer, np.floating)
        for name, v in (("reflectivity", reflectivity), ("f0", f0)):
            if isinstance(v, bool) or not isinstance(v, number) or not 0 <= float(v) <= 1:
                raise ValueError(f"{name} must be a number from 0 to 1, got {v!r}")
        try:
            tint3 = [float(v) for v in tint]
        except (TypeError, ValueError):
            tint3 = []
        if len(tint3) != 3 or not np.isfinite(np.float32(tint3)).all():
            raise ValueError(f"tint must be three finite numbers, got {tint!r}")
        if isinstance(level, bool) or not isinstance(level, number) or not float(level) >= 0:
            raise ValueError(f"level must be a number, 0 or above, got {level!r}")
        M = np.eye(3, dtype=np.float32) if orientation is None else np.asarray(orientation, dtype=np.float32)
        if M.shape != (3, 3) or not np.isfinite(M).all():
            raise ValueError(f"orientation must be None or a finite 3 x 3 matrix, got {orientation!r}")
        if background is None or background is False:
            gain = None
        elif background is True:
            gain = 1.0
        elif isinstance(background, number) and np.isfinite(np.float32(background)) and float(background) >= 0:
            gain = float(background)
        else:
            raise ValueError(f"background must be None, a bool or a finite gain, 0 or above, got {background!r}")
        self._pass_target("environment_pass")
        if self._environment is None:
            raise ValueError("environment_pass: no environment is bound (bind_environment)")
        cube, chain = self._environment
        sides = self.environment_levels()
        lam = float(level)
        if lam > 0 and chain is None:
            raise ValueError(f"level={level!r} needs a mip chain: bind_environment(..., mipmaps=True)")
        if lam > len(sides) - 1:
            raise ValueError(f"level must be at most {len(sides) - 1}, the last level of the bound chain, got {level!r}")
        tri, T = self._pass_frame("environment_pass")
        if float(reflectivity) == 0 and gain is None:
            return
        l0 = int(np.floor(lam))
        f = float(np.float32(lam - l0))
        if f >= 1.0:                    # (a fraction that rounds up to the next level)
            l0, f = l0 + 1, 0.0
        if l0 == len(sides) - 1:
            f = 0.0
        two = f != 0.0
        faces0 = cube if chain is None else chain[0][chain[2][l0]:]
        faces1 = chain[0][chain[2][l0 + 1]:] if two else None
        flags = _capi.ENV_REFLECT | (_capi.ENV_BACKGROUND if gain is not None else 0)
        self._run_pass("crender_env_shade", tri, T,
                       (self.normals_buffer, faces0, sides[l0], faces1, sides[l0 + 1] if two else 0, f,
                        (C.c_float * 9)(*[float(v) for v in M.reshape(9)]), float(reflectivity), float(f0),
                        (C.c_float * 3)(*tint3), 0.0 if gain is None else gain), flags)

    def bind_shadow_map(self, light_filler, light_vertices):
        """Name the shadow map of ``shadow_pass``: `light_filler`, another ``AdvancedPixelBufferFiller`` on the same
        device (not a swap chain) into which the SAME triangles are rendered from the light, and `light_vertices`
        float32 [T, 3, 3], numpy or a device tensor, in the caller's triangle order: the vertex array that filler
        was given to draw (``shadow.light_arrays``).  The binding holds the filler object; its planes are read when
        the pass runs.  ``bind_shadow_map(None, None)`` drops the binding."""
        if light_filler is None and light_vertices is None:
            self._shadow = None
            return
        if light_filler is None or light_vertices is None:
            raise ValueError("bind_shadow_map needs both the light's filler and its vertices (or None, None)")
        if not isinstance(light_filler, DeferredPasses):
            raise ValueError(f"bind_shadow_map: the light's filler must be an AdvancedPixelBufferFiller, "
                             f"got {type(light_filler).__name__}")
        if light_filler._pipeline:
            raise ValueError("bind_shadow_map: the light's filler is a swap chain (pipeline=True): its planes rotate")
        if light_filler.device != self.device:
            raise ValueError(f"bind_shadow_map: the light's filler is on {light_filler.device}, this one on {self.device}")
        self._shadow = (light_filler, _as_device_f32(light_vertices, "light_vertices", self.device))

    def shadow_pass(self, bias=1e-3, pcf=1, ambient=0.25, use_winner=True):
        """Shadow mapping of the LAST frame's colour plane (``crender_shadow_shade``, include/crender_shadow.h)
        against the last frame of the filler bound with ``bind_shadow_map``: the surface point every covered pixel
        shows is carried into the light's frame (perspective-correct) and projected into the light's z plane; the
        pixel is shadowed where that plane holds something nearer by more than `bias` (in the light's projected z).
        `pcf` K = 1, 3 or 5 averages the K x K texels around it; a fully shadowed pixel keeps `ambient` of its
        colour, a fully lit one is not written at all.  With `use_winner` and a light filler that tracks its winner
        plane, a texel the pixel's own triangle won is lit whatever the depths say, which removes the self-shadowing
        of a surface on itself without a bias.  Rows of the filler's ``row_strip``, on torch's current stream.

        Both frames are settled first (one stream synchronisation each, as every getter does): a frame whose bin
        lists overflowed is rendered again, the pass must land on the camera frame that stays and see the light's
        final z."""
        self._pass_target("shadow_pass")
        if self._shadow is None:
            raise ValueError("shadow_pass: no shadow map is bound (bind_shadow_map)")
        light, ltri = self._shadow
        tri, T = self._pass_frame("shadow_pass", "the camera's filler")
        drawn = light._pass_frame("shadow_pass", "the light's filler")[1]
        if not ltri.shape[0] == drawn == T:
            raise ValueError(f"shadow_pass: {ltri.shape[0]} triangles of light-frame vertices are bound, the light's last "
                             f"frame drew {drawn}, the camera's {T}")
        if isinstance(pcf, bool) or pcf not in _capi.SHADOW_PCF:
            raise ValueError(f"pcf must be 1, 3 or 5, got {pcf!r}")
        self._run_pass("crender_shadow_shade", tri, T,
                       (ltri if T else None, light._P, light.z_buffer, light.winner_buffer if use_winner else None,
                        light.h, light.w, float(bias), float(ambient), int(pcf)), light=light)

    def phong_pass(self, lights, ambient=0.1, shininess=32, specular_color=(255, 255, 255), clamp=255.0):
        """Per-pixel Blinn-Phong lighting of the LAST frame's colour plane (``crender_phong_shade``,
        include/crender_phong.h): every covered pixel's colour c becomes ``min(c * F + Ws * specular_color, clamp)``
        with ``F = ambient + sum kd_j * d_j`` and ``Ws = sum ks_j * sp_j ** shininess`` over the lights, d_j the
        Guro factor of the pixel's stored normal under the unit vector towards light j, sp_j that of the half vector
        between it and the direction to the camera, both taken at the surface point the pixel shows (the
        perspective-correct blend of the winner's corners).  `lights` is a list of 1 to 4 dicts, each with exactly one
        of ``position`` (a point in the camera's frame, where ``shadow.look_at(position=...)`` places a light) or
        ``direction`` (the way the light travels, ``GuroIllumination``'s convention: flipped and normalised by that
        class's own statements), and ``diffuse`` (kd) and ``specular`` (ks).  `shininess` is a power of two from 1 to
        4096.  The background is not written.  Rows of the filler's ``row_strip``, on torch's current stream.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin lists
        overflowed is rendered again, and the pass must land on the frame that stays."""
        from ..illumination.phong_illumination import light_rows, shininess_log2
        self._pass_target("phong_pass")
        rows, mask = light_rows(lights)
        k = shininess_log2(shininess)
        tri, T = self._pass_frame("phong_pass")
        lights5 = (C.c_float * (5 * len(rows)))(*[v for row in rows for v in row])
        spec = (C.c_float * 3)(*[float(v) for v in specular_color])
        self._run_pass("crender_phong_shade", tri, T,
                       (self.normals_buffer, lights5, len(rows), mask, float(ambient), k, spec, float(clamp)))

    def ao_pass(self, radius=0.03, radius_px=8, taps=16, min_cos=0.1, strength=2.0, floor=0.0, rotate=True, normals="plane"):
        """Screen-space ambient occlusion of the LAST frame's colour plane (``crender_ao_shade``,
        include/crender_ao.h): every covered pixel's colour is scaled by ``max(1 - strength * mean(o_i), floor)``,
        where tap i looks at the covered pixel at its offset, takes the point that pixel shows (from the z plane) and
        gives ``o_i = cos * (1 - (distance / radius) ** 2)`` if the point lies within `radius` (in the camera frame's
        units) and the cosine between the pixel's normal and the way to it exceeds `min_cos`, else 0.  `taps` is a
        count — the table ``ambient_occlusion.taps(radius_px, taps)`` — or an explicit list of (dx, dy) pairs, 1 to 64
        of them within `radius_px` (1 to 32) in both coordinates.  With `rotate` a pixel turns the table by a quarter
        turn picked by its parity, so that neighbours look in other directions.  `normals` is ``"plane"`` (the normal
        plane the raster stored: interpolated vertex normals) or ``"face"`` (the winner's own geometric normal, turned
        to the eye).  A pixel that nothing occludes is not written.  Rows of the filler's ``row_strip``, on torch's
        current stream; the strip does not see across its edge.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin lists
        overflowed is rendered again, and the pass must land on the frame that stays."""
        from .. import ambient_occlusion
        self._pass_target("ao_pass")
        if normals not in ("plane", "face"):
            raise ValueError(f"normals must be 'plane' or 'face', got {normals!r}")
        if isinstance(radius_px, bool) or not isinstance(radius_px, int) or not 1 <= radius_px <= _capi.AO_MAX_RADIUS_PX:
            raise ValueError(f"radius_px must be an int from 1 to {_capi.AO_MAX_RADIUS_PX}, got {radius_px!r}")
        if isinstance(taps, int) and not isinstance(taps, bool):
            if not 1 <= taps <= _capi.AO_MAX_TAPS:
                raise ValueError(f"taps must be a count from 1 to {_capi.AO_MAX_TAPS} or a list of (dx, dy) pairs, got {taps!r}")
            table = ambient_occlusion.taps(radius_px, taps)
        else:
            try:
                table = [(operator.index(dx), operator.index(dy)) for dx, dy in taps]
            except (TypeError, ValueError):
                raise ValueError(f"taps must be a count from 1 to {_capi.AO_MAX_TAPS} or a list of (dx, dy) pairs, "
                                 f"got {taps!r}") from None
            if not 1 <= len(table) <= _capi.AO_MAX_TAPS:
                raise ValueError(f"taps must hold 1 to {_capi.AO_MAX_TAPS} pairs, got {len(table)}")
            for dx, dy in table:
                if max(abs(dx), abs(dy)) > radius_px or (dx, dy) == (0, 0):
                    raise ValueError(f"the tap ({dx}, {dy}) is (0, 0) or reaches beyond radius_px={radius_px}")
        tri, T = self._pass_frame("ao_pass")
        taps2 = (C.c_int8 * (2 * len(table)))(*[v for pair in table for v in pair])
        flags = (_capi.AO_ROTATE if rotate else 0) | (_capi.AO_FACE_NORMALS if normals == "face" else 0)
        self._run_pass("crender_ao_shade", tri, T, (self.normals_buffer, taps2, len(table), radius_px, float(radius),
                                                    float(min_cos), float(strength), float(floor)), flags, z=True)

    def wire_pass(self, width=1.0, color=(255, 255, 255), feather=1.0, opacity=1.0, fill=None, edges=None, outline=False,
                  depth_bias=1e-3, radius_px=None):
        """A hidden-line wireframe over the LAST frame's colour plane (``crender_wire_overlay``,
        include/crender_wire.h): every covered pixel takes its distance in pixels to the nearest drawn edge of the
        triangle that WON it, and is blended towards `color` by ``opacity * clip((width / 2 + feather / 2 - distance) /
        feather, 0, 1)``.  A line behind a nearer triangle is never drawn, since its pixels name the nearer triangle:
        no depth bias.  With `fill` (a colour) every covered pixel is first given that colour — lines on a flat body,
        a hidden-line drawing; without it the lines lie over the shaded surface and a pixel off every line is not
        written.  `edges` is None (all three edges of every triangle) or a uint8 array [T], numpy or a device tensor,
        in the caller's triangle order: bit e of entry t draws the edge from corner e to corner (e + 1) % 3
        (``wireframe.feature_edges`` picks creases and borders).  `width` and `feather` are in pixels, in (0, 64];
        `opacity` in [0, 1].  The background is not written.  Rows of the filler's ``row_strip``, on torch's current
        stream.

        With `outline` (``crender_wire_outline``) the lines have their full width: a pixel takes its distance to the
        nearest drawn edge SEGMENT of every triangle that won a pixel within `radius_px` of it (0 to 8; None:
        ``ceil((width + feather) / 2) + 1``, which holds a whole line and so limits ``width + feather`` to 14), the strip
        not seeing across its edge.  The outer half of a silhouette, a border or an occlusion boundary is then drawn as
        well, with its ramp: on the background, which is written only where a line lies and never filled, and on a
        farther surface, where an edge counts if its projected depth at its closest point, less `depth_bias` (in the z
        plane's units, as ``shadow_pass``'s bias), is nearer than what the pixel shows.  A line behind the surface a
        pixel shows is not drawn.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin lists
        overflowed is rendered again, and the pass must land on the frame that stays."""
        self._pass_target("wire_pass")
        for name, v in (("width", width), ("feather", feather)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 < float(v) <= _capi.WIRE_MAX_WIDTH:
                raise ValueError(f"{name} must be a number of pixels above 0 and at most {_capi.WIRE_MAX_WIDTH}, got {v!r}")
        if isinstance(opacity, bool) or not isinstance(opacity, (int, float, np.integer, np.floating)) or not 0 <= float(opacity) <= 1:
            raise ValueError(f"opacity must be a number from 0 to 1, got {opacity!r}")
        if outline:
            top = _capi.WIRE_OUTLINE_MAX_RADIUS
            if isinstance(depth_bias, bool) or not isinstance(depth_bias, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(float(depth_bias)):
                raise ValueError(f"depth_bias must be a finite number, got {depth_bias!r}")
            if radius_px is None:
                radius_px = int(np.ceil((float(width) + float(feather)) / 2.0)) + 1
                if radius_px > top:
                    raise ValueError(f"outline=True: width + feather = {float(width) + float(feather):g} needs radius_px = "
                                     f"{radius_px}, above the largest, {top}: width + feather may be at most {2 * (top - 1)}")
            elif isinstance(radius_px, bool) or not isinstance(radius_px, (int, np.integer)) or not 0 <= radius_px <= top:
                raise ValueError(f"radius_px must be None or an int from 0 to {top}, got {radius_px!r}")
        tri, T = self._pass_frame("wire_pass")
        edges = _edge_mask(self, edges, T)
        line3 = (C.c_float * 3)(*[float(v) for v in color])
        fill3 = None if fill is None else (C.c_float * 3)(*[float(v) for v in fill])
        if outline:
            self._run_pass("crender_wire_outline", tri, T,
                           (edges if T else None, line3, fill3, float(width), float(feather), float(opacity),
                            float(depth_bias), int(radius_px)), z=True)
            return
        self._run_pass("crender_wire_overlay", tri, T,
                       (edges if T else None, line3, fill3, float(width), float(feather), float(opacity)))

    def hidden_line_pass(self, color=(0, 0, 0), opacity=0.5, dash=(4, 4), edges=None, depth_bias=1e-3, use_winner=True):
        """The edges BEHIND the surface, dashed, over the LAST frame's colour plane (``crender_wire_hidden``,
        include/crender_wire.h): the far side of a technical drawing, which ``wire_pass`` cannot show, since it sees an
        edge only through pixels the edge's own triangle won.  Every drawn half-edge is projected, rounded to pixel
        centres and walked with the wireframe filler's Bresenham; a step is hidden where the z plane holds something
        nearer than the edge's own depth there, less `depth_bias` (in the z plane's units, as ``wire_pass``'s), and —
        with `use_winner` — the pixel was not won by the edge's own triangle.  A pixel through which a hidden edge runs,
        and no drawn edge that is visible there, is blended towards `color` by `opacity` (0 to 1) if its coordinate
        along the edge's major axis falls into the first ``dash[0]`` (1 to 64) pixels of every ``dash[0] + dash[1]``
        (``dash[1]`` 0 to 64; 0 is a solid line): one pixel wide, the pattern anchored to the screen.  `edges` is
        ``wire_pass``'s: None or a uint8 array [T] in the caller's triangle order (``wireframe.feature_edges``,
        ``contour_edges``).  Rows of the filler's ``row_strip``, on torch's current stream.  The pass keeps a zeroed
        int32 [h, w] key plane on the device, allocated at the first call.

        The frame is settled first (one stream synchronisation, as every getter does): a frame whose bin lists
        overflowed is rendered again, and the pass must land on the frame that stays."""
        self._pass_target("hidden_line_pass")
        number = (int, float, np.integer, np.floating)
        if isinstance(opacity, bool) or not isinstance(opacity, number) or not 0 <= float(opacity) <= 1:
            raise ValueError(f"opacity must be a number from 0 to 1, got {opacity!r}")
        top = _capi.WIRE_MAX_DASH
        try:
            on, off = dash
            bad = any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (on, off))
        except (TypeError, ValueError):
            bad = True
        if bad or not 1 <= on <= top or not 0 <= off <= top:
            raise ValueError(f"dash must be a pair of ints (on, off) with on from 1 to {top} and off from 0 to {top}, got {dash!r}")
        if isinstance(depth_bias, bool) or not isinstance(depth_bias, number) or not np.isfinite(float(depth_bias)):
            raise ValueError(f"depth_bias must be a finite number, got {depth_bias!r}")
        try:
            line = [float(v) for v in color]
        except (TypeError, ValueError):
            line = []
        if len(line) != 3 or not np.isfinite(line).all():
            raise ValueError(f"color must be three finite numbers, got {color!r}")
        tri, T = self._pass_frame("hidden_line_pass")
        edges = _edge_mask(self, edges, T)
        if self._hidden_key is None:
            self._hidden_key = torch.zeros((self.h, self.w), dtype=torch.int32, device=self.color_buffer.device)
        self._run_pass("crender_wire_hidden", tri, T,
                       (edges if T else None, (C.c_float * 3)(*line), float(opacity), int(on), int(off), float(depth_bias),
                        self._hidden_key), _capi.WIRE_HIDDEN_USE_WINNER if use_winner else 0, z=True)

    def line_runs(self, edges=None, partners=None, depth_bias=1e-3, use_winner=True):
        """The hidden-line drawing of the LAST frame as vector segments (``crender_wire_runs_count`` and
        ``crender_wire_runs_emit``, include/crender_wire.h): a ``LineDrawing``.  Every drawn half-edge is projected, rounded
        and walked as ``hidden_line_pass`` walks it, and every step is classed hidden or visible by the same test against
        the z plane; the steps are then joined into maximal runs of one class per edge, and every run comes back as a
        sub-segment of the edge's unrounded projection, in the frame's pixel coordinates and clipped to the frame:
        ``drawing.runs`` int32 [N, 4] holds (segment 3 i + e, first step, last step, class: 1 hidden, 2 visible) and
        ``drawing.ends`` float32 [N, 4] (x0, y0, x1, y1), ordered by (segment, first step), device tensors both.
        `edges` is ``hidden_line_pass``'s mask; a vector drawing wants every mesh edge ONCE: ``wireframe.half_edges_once``.
        `partners` (None, or the int32 [T, 3] table of ``wireframe.edge_partners``, numpy or a device tensor) extends the
        winner rule of `use_winner` to the triangle across the edge: a step is visible where either of the edge's two
        triangles won the pixel.  ``wireframe.write_svg`` writes the drawing.  Rows of the filler's ``row_strip``, on
        torch's current stream.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The call then counts, reads the total ONCE (``.item()``: its one
        extra synchronisation; the size of the result is not known before) and stores.  The planes are only read: the
        views stay as fresh or as stale as they were."""
        self._pass_target("line_runs")
        if isinstance(depth_bias, bool) or not isinstance(depth_bias, (int, float, np.integer, np.floating)) \
                or not np.isfinite(float(depth_bias)):
            raise ValueError(f"depth_bias must be a finite number, got {depth_bias!r}")
        tri, T = self._pass_frame("line_runs")
        edges = _edge_mask(self, edges, T)
        if partners is not None:
            partners = _device_array(self, partners, torch.int32, lambda s: len(s) == 2 and s[1] == 3,
                                     "partners must be int32 [T, 3] (wireframe.edge_partners)")
            if partners.shape[0] != T:
                raise ValueError(f"line_runs: the partner table holds {partners.shape[0]} triangles, the last frame drew {T}")
        if 3 * T > 2 ** 31 - 1:
            raise ValueError(f"line_runs takes at most {(2 ** 31 - 1) // 3} triangles, the last frame drew {T}")
        self._push_host_edits()
        self._check_bins()
        device = self.color_buffer.device
        groups = -(-3 * T // _capi.WIRE_RUNS_GROUP)
        runs = torch.empty((0, 4), dtype=torch.int32, device=device)
        ends = torch.empty((0, 4), dtype=torch.float32, device=device)
        if groups == 0:
            return LineDrawing(runs, ends, self.h, self.w)
        pos_of = None if self._order is None else self._order[1]
        flags = _capi.WIRE_RUNS_USE_WINNER if use_winner else 0
        head = (self.winner_buffer, self.z_buffer, tri, T, pos_of, self._P, edges, partners, float(depth_bias))
        tail = (self.h, self.w, self.y0, self.y1, flags)
        counts = torch.empty(groups, dtype=torch.int32, device=device)       # (a uint32 below 2^28: the same bits)
        self._launch_pass("crender_wire_runs_count", head + (counts,) + tail)
        after = torch.cumsum(counts, 0, dtype=torch.int64)
        N = int(after[-1].item())
        if N:
            runs = torch.empty((N, 4), dtype=torch.int32, device=device)
            ends = torch.empty((N, 4), dtype=torch.float32, device=device)
            self._launch_pass("crender_wire_runs_emit", head + (after - counts, N, runs, ends) + tail)
        return LineDrawing(runs, ends, self.h, self.w)

    def edge_aa(self, edges=None):
        """Geometric edge anti-aliasing of the LAST frame (``crender_wire_edge_aa``, include/crender_wire.h): a NEW
        device tensor [h, w, 3] float32, as ``resolve`` returns one, in which every pixel whose left, right, upper or
        lower neighbour shows another triangle is blended with ONE of those neighbours by the share of its cell that
        lies beyond the edge between them.  The edge is the nearer triangle's (by the z plane), and where it crosses
        the line between the two pixel centres comes from the rasterizer's own barycentrics: coverage computed, not
        sampled, at the frame's own resolution.  Every other pixel is copied bit for bit.  `edges` is ``wire_pass``'s:
        None (every edge smooths) or a uint8 array [T], numpy or a device tensor, in the caller's triangle order —
        ``contour_edges(partners, static=feature_edges(...), borders=True)`` names the contours, creases and borders
        of a view and leaves the Gouraud-shaded interior of a smooth surface alone.  Rows of the filler's
        ``row_strip`` (the others of the result are zero; the strip does not see across its edge), on torch's current
        stream.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes are only read: the views stay as fresh or as stale
        as they were."""
        self._pass_target("edge_aa")
        tri, T = self._pass_frame("edge_aa")
        edges = _edge_mask(self, edges, T)
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        out = new((self.h, self.w, 3), dtype=torch.float32, device=self.color_buffer.device)
        self._run_pass("crender_wire_edge_aa", tri, T, (edges if T else None, out), z=True, reads_only=True)
        return out

    def depth_of_field(self, focus, aperture=4.0, band=0.0, max_radius=8):
        """Depth of field of the LAST frame (``crender_dof_blur``, include/crender_dof.h): a NEW device tensor [h, w, 3]
        float32, as ``edge_aa`` returns one, in which every pixel is the weighted mean of the pixels around it, each
        weighted by how far its own circle of confusion reaches.  A covered pixel at view depth zv (rebuilt from the z
        plane; ``depth_of_field.view_depth`` gives the same number, so ``focus=view_depth(filler._P, z[y, x])`` focuses
        on what a pixel shows) has the radius ``aperture * (|zv - focus| - band)+ / zv`` pixels — nothing within `band`
        of `focus` is blurred, and `aperture` is the radius at infinity, which the background has — clamped to
        `max_radius` (an int from 1 to 12), which is also how far a pixel looks.  What is in front spreads over what
        lies behind it by its own radius; a blurred background does not bleed over something sharper in front of it.
        ``aperture=0`` and every pixel that no blurred one reaches are copied bit for bit.  Rows of the filler's
        ``row_strip`` (the others of the result are zero; the strip does not see across its edge), on torch's current
        stream.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes are only read: the views stay as fresh or as stale
        as they were."""
        self._pass_target("depth_of_field")
        tri, T = self._pass_frame("depth_of_field")
        number = (int, float, np.integer, np.floating)
        top32 = float(np.finfo(np.float32).max)        # (finite as the float32 the library takes)
        if isinstance(focus, bool) or not isinstance(focus, number) or not 0 < float(focus) <= top32 or not np.float32(focus) > 0:
            raise ValueError(f"focus must be a finite view depth above 0, got {focus!r}")
        for name, v in (("aperture", aperture), ("band", band)):
            if isinstance(v, bool) or not isinstance(v, number) or not 0 <= float(v) <= top32:
                raise ValueError(f"{name} must be a finite number, 0 or above, got {v!r}")
        top = _capi.DOF_MAX_RADIUS
        if isinstance(max_radius, bool) or not isinstance(max_radius, (int, np.integer)) or not 1 <= max_radius <= top:
            raise ValueError(f"max_radius must be an int from 1 to {top}, got {max_radius!r}")
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        out = new((self.h, self.w, 3), dtype=torch.float32, device=self.color_buffer.device)
        self._run_pass("crender_dof_blur", tri, T, (self.color_buffer, float(focus), float(band), float(aperture),
                                                    int(max_radius)), z=True, reads_only=True, target=out)
        return out

    def _previous_pose(self, name, previous_vertices, T):
        """`previous_vertices` as ``bind_shadow_map`` converts ``light_vertices``; it must hold the last frame's T triangles."""
        if previous_vertices is None:
            raise ValueError(f"{name}: previous_vertices is None: the vertex array of the earlier pose is needed")
        prev = _as_device_f32(previous_vertices, "previous_vertices", self.device)
        if prev.shape[0] != T:
            raise ValueError(f"{name}: previous_vertices holds {prev.shape[0]} triangles, the last frame drew {T}")
        return prev

    @staticmethod
    def _check_exposure(exposure):
        if isinstance(exposure, bool) or not isinstance(exposure, (int, float, np.integer, np.floating)) \
                or not 0 <= float(exposure) <= float(np.finfo(np.float32).max):
            raise ValueError(f"exposure must be a finite number, 0 or above, got {exposure!r}")

    def motion_vectors(self, previous_vertices, exposure=1.0):
        """The motion vectors of the LAST frame against an earlier pose (``crender_motion_vectors``,
        include/crender_motion.h): a NEW device tensor [h, w, 2] float32 in which a covered pixel holds (vx, vy), the
        pixels the surface point it shows moved on the screen between the pose of `previous_vertices` and the frame's,
        times `exposure` — pointing from where it was to where it is.  The point is the perspective-correct blend of the
        winner's three PREVIOUS corners with the rasterizer's own barycentrics, projected with the filler's own matrix,
        as ``shadow_pass`` carries it into the light's frame: exact per pixel, no finite differences.
        `previous_vertices` is float32 [T, 3, 3], numpy or a device tensor, in the caller's triangle order and in the
        camera's frame: the vertex array of the earlier pose, T the triangles of the last frame.  The background, a
        point that was behind the camera and a velocity that is not finite give (0, 0).  Rows of the filler's
        ``row_strip`` (the others of the result are zero), on torch's current stream.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes are only read: the views stay as fresh or as stale
        as they were."""
        self._pass_target("motion_vectors")
        tri, T = self._pass_frame("motion_vectors")
        prev = self._previous_pose("motion_vectors", previous_vertices, T)
        self._check_exposure(exposure)
        return self._motion_vectors(tri, T, prev, exposure)

    def _motion_vectors(self, tri, T, prev, exposure):
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        out = new((self.h, self.w, 2), dtype=torch.float32, device=self.color_buffer.device)
        self._run_pass("crender_motion_vectors", tri, T, (prev if T else None, float(exposure)), reads_only=True, target=out)
        return out

    def motion_blur(self, previous_vertices=None, *, velocity=None, exposure=1.0, max_radius=8, taps=16, soft=0.02):
        """Motion blur of the LAST frame (``crender_motion_blur``, include/crender_motion.h): a NEW device tensor
        [h, w, 3] float32, as ``depth_of_field`` returns one, in which every pixel is the weighted mean of `taps` pixels
        on a line through it: the reconstruction filter of McGuire et al. 2012.  The line is the DOMINANT half velocity
        of the pixel's tile of 32 x 32 and of `max_radius` pixels around it (an int from 1 to 12: every half velocity is
        clamped to it), and a tap counts by the two pixels' velocities and view depths: what moves spreads over what
        lies behind it, what stands still in front of something moving keeps its bits, and depths closer than `soft`
        blend.  The velocities come from `previous_vertices` (``motion_vectors``' argument, with `exposure`) or from
        `velocity`, a float32 [h, w, 2] array or tensor such as an edited result of ``motion_vectors``: exactly one of
        the two.  A tile in which nothing moves by more than a pixel, and every pixel that takes no tap, is copied bit
        for bit.  Rows of the filler's ``row_strip`` (the others of the result are zero; the strip does not see across
        its edge), on torch's current stream.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes are only read: the views stay as fresh or as stale
        as they were."""
        self._pass_target("motion_blur")
        tri, T = self._pass_frame("motion_blur")
        if (previous_vertices is None) == (velocity is None):
            raise ValueError("motion_blur takes exactly one of previous_vertices and velocity")
        self._check_exposure(exposure)
        top = _capi.MOTION_MAX_RADIUS
        if isinstance(max_radius, bool) or not isinstance(max_radius, (int, np.integer)) or not 1 <= max_radius <= top:
            raise ValueError(f"max_radius must be an int from 1 to {top}, got {max_radius!r}")
        top = _capi.MOTION_MAX_TAPS
        if isinstance(taps, bool) or not isinstance(taps, (int, np.integer)) or not 1 <= taps <= top:
            raise ValueError(f"taps must be an int from 1 to {top}, got {taps!r}")
        if isinstance(soft, bool) or not isinstance(soft, (int, float, np.integer, np.floating)) \
                or not 0 < float(soft) <= float(np.finfo(np.float32).max) or not np.float32(soft) > 0:
            raise ValueError(f"soft must be a finite range of view depths above 0, got {soft!r}")
        if velocity is not None:
            if float(exposure) != 1.0:
                raise ValueError(f"exposure={exposure!r} with velocity=...: the exposure scales the velocities "
                                 "motion_vectors computes; scale the plane itself")
            velocity = _device_array(self, velocity, torch.float32, lambda s: s == (self.h, self.w, 2),
                                     f"velocity must be float32 [{self.h}, {self.w}, 2], the frame's")
        else:
            velocity = self._motion_vectors(tri, T, self._previous_pose("motion_blur", previous_vertices, T), exposure)
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        out = new((self.h, self.w, 3), dtype=torch.float32, device=self.color_buffer.device)
        self._run_pass("crender_motion_blur", tri, T, (self.color_buffer, velocity, int(max_radius), int(taps), float(soft)),
                       z=True, reads_only=True, target=out)
        return out

    def temporal_resolve(self, history, previous_vertices=None, *, velocity=None, blend=0.1, dilate=True, clamp=True):
        """Temporal anti-aliasing of the LAST frame (``crender_taa_resolve``, include/crender_taa.h): a NEW device tensor
        [h, w, 3] float32, as ``edge_aa`` returns one, in which every pixel is ``c + (hist - c) * (1 - blend)``: its own
        colour c blended towards `history` (float32 [h, w, 3], numpy or a device tensor: the image this method returned
        for the frame before) sampled bilinearly where the surface point the pixel shows WAS, and, with `clamp`, clamped
        per channel to the range of the frame's colours in the pixel's 3 x 3 first, which keeps a stale history from
        ghosting.  Where it was comes from `previous_vertices` (``motion_vectors``' argument, at exposure 1) or from
        `velocity`, a float32 [h, w, 2] array or tensor such as an edited result of ``motion_vectors``: at most one of
        the two, and neither means a static view (no velocity plane is made or read).  With `dilate` the velocity is
        taken from the nearest pixel of the 3 x 3 by the z plane, so that a silhouette carries its own motion over the
        background pixels it is blended into; it is ignored without a velocity.  `blend` is the new frame's share, in
        (0, 1]; 1 returns the frame's rows, copied, and so does ``history=None``.  A pixel whose previous position is off
        the frame (or outside the strip) keeps its own colour.  Rows of the filler's ``row_strip`` (the others of the
        result are zero; the strip does not see across its edge), on torch's current stream.  Draw the frames with a
        sub-pixel offset each (``temporal.jitter_offsets``, ``view_shear``, ``sheared``) and the image converges towards
        the supersampled one; ``Renderer(temporal_aa=...)`` does both.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes and the history are only read: the views stay as fresh
        or as stale as they were."""
        self._pass_target("temporal_resolve")
        tri, T = self._pass_frame("temporal_resolve")
        if previous_vertices is not None and velocity is not None:
            raise ValueError("temporal_resolve takes at most one of previous_vertices and velocity")
        if isinstance(blend, bool) or not isinstance(blend, (int, float, np.integer, np.floating)) \
                or not 0 < float(blend) <= 1 or not np.float32(blend) > 0:
            raise ValueError(f"blend must be a number above 0 and at most 1, got {blend!r}")
        for name, v in (("dilate", dilate), ("clamp", clamp)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"{name} must be a bool, got {v!r}")
        if history is not None:
            history = _device_array(self, history, torch.float32, lambda s: s == (self.h, self.w, 3),
                                    f"history must be None or float32 [{self.h}, {self.w}, 3], the frame's")
        if velocity is not None:
            velocity = _device_array(self, velocity, torch.float32, lambda s: s == (self.h, self.w, 2),
                                     f"velocity must be float32 [{self.h}, {self.w}, 2], the frame's")
        elif previous_vertices is not None:
            prev = self._previous_pose("temporal_resolve", previous_vertices, T)
            if history is not None:
                velocity = self._motion_vectors(tri, T, prev, 1.0)
        self._push_host_edits()
        self._check_bins()
        whole = (self.y0, self.y1) == (0, self.h)
        out = (torch.empty if whole else torch.zeros)((self.h, self.w, 3), dtype=torch.float32, device=self.color_buffer.device)
        if history is None:
            out[self.y0:self.y1].copy_(self.color_buffer[self.y0:self.y1])
            return out
        flags = 0 if clamp else _capi.TAA_NO_CLAMP
        self._launch_pass("crender_taa_resolve", (self.color_buffer, history, velocity,
                                                  self.z_buffer if dilate and velocity is not None else None,
                                                  float(np.float32(blend)), out, self.h, self.w, self.y0, self.y1, flags))
        return out

    def _peel_frame(self, name):
        """What the two transparency methods share: the refusals and the frame of ``edge_aa``, the edits pushed and the
        frame settled; -> (tri, col, nrm or None each, T, pos_of, the cached scratch)."""
        self._pass_target(name)
        tri, T = self._pass_frame(name)
        self._push_host_edits()
        self._check_bins()
        if self._peel_scratch is None:
            device = self.color_buffer.device
            self._peel_scratch = (
                torch.empty((self.h, self.w), dtype=torch.int64, device=device),     # crender_atomic_scratch_bytes(h, w)
                torch.empty((self.h, self.w), dtype=torch.float32, device=device),   # the transmittance
                torch.empty((2, self.h, self.w), dtype=torch.int32, device=device),  # two winner planes and
                torch.empty((2, self.h, self.w), dtype=torch.float32, device=device))  # two z planes, used in turn
        pos_of = None if self._order is None else self._order[1]
        arrays = tuple(self._inputs[:3]) if T else (None, None, None)
        return arrays + (T, pos_of, self._peel_scratch)

    def peel_layers(self, n):
        """The first `n` (1 to 16) depth layers of the LAST frame (``crender_peel_next``, include/crender_peel.h):
        ``(winner int32 [n, h, w], z float32 [n, h, w])``, device tensors.  Layer 0 is a copy of the frame's own winner and
        z planes; layer k + 1 names, per pixel, the fragment of the frame with the least depth key strictly above layer
        k's — the next surface behind it, coplanar duplicates one by one, the highest index first — with that fragment's
        own z, or -1 and 1e6 where nothing lies behind.  The frame's back-face culling applies to every layer.  Rows of
        the filler's ``row_strip`` (the others of the result are zero), on torch's current stream.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes are only read: the views stay as fresh or as stale
        as they were.  The scratch (8 bytes of key a pixel, and ``transparency_pass``'s 20) is allocated at the first call and
        kept."""
        top = _capi.PEEL_MAX_LAYERS
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= top:
            raise ValueError(f"n must be an int from 1 to {top}, got {n!r}")
        tri, _, nrm, T, pos_of, (keys, _, _, _) = self._peel_frame("peel_layers")
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        device = self.color_buffer.device
        winner = new((int(n), self.h, self.w), dtype=torch.int32, device=device)
        z = new((int(n), self.h, self.w), dtype=torch.float32, device=device)
        rows = slice(self.y0, self.y1)
        winner[0, rows].copy_(self.winner_buffer[rows])
        z[0, rows].copy_(self.z_buffer[rows])
        for k in range(1, int(n)):
            self._launch_pass("crender_peel_next", (winner[k - 1], z[k - 1], tri, T, pos_of, self._P, nrm, keys, winner[k],
                                                    z[k], self.h, self.w, self.y0, self.y1, 0))
        return winner, z

    def transparency_pass(self, alpha, layers=4, light_direction=None, background=(0, 0, 0), front="plane"):
        """The LAST frame with its triangles transparent (``crender_peel_next`` and ``crender_peel_blend``,
        include/crender_peel.h): a NEW device tensor [h, w, 3] float32, as ``edge_aa`` returns one.  The first `layers` (1 to
        16) depth layers of every pixel are peeled as ``peel_layers`` peels them and blended front to back: a layer adds
        ``transmittance * alpha * colour`` and leaves ``transmittance * (1 - alpha)``, and what is left after the last one
        shows `background` (three finite numbers).  `alpha` is a number, or an array [T] in the caller's triangle order,
        numpy (checked: values outside [0, 1] and NaN raise) or a float32 device tensor (clamped on the device, a NaN is
        0).  ``front="plane"`` takes layer 0's colours from the filler's colour plane, so whatever the other passes made
        of the visible surface is kept; ``front="model"`` shades it from the triangle's vertex colours like the layers
        behind it, which are lit by `light_direction` (the illumination object's own flipped, normalised vector, as
        ``set_fused_illumination`` takes it) if it is given.  A pixel that has become opaque is not touched again.
        ``alpha=1`` with ``front="plane"`` returns the colour plane's bits over the background.  Rows of the filler's
        ``row_strip`` (the others of the result are zero), on torch's current stream: `layers` blends and
        ``layers - 1`` peels over two pairs of planes used in turn, without a host synchronisation between them.

        Edits made in the numpy views handed out so far are carried to the device and the frame is settled first (one
        stream synchronisation, as every getter does).  The planes are only read: the views stay as fresh or as stale
        as they were.  The scratch (28 bytes a pixel, shared with ``peel_layers``) is allocated at the first call and kept."""
        top = _capi.PEEL_MAX_LAYERS
        number = (int, float, np.integer, np.floating)
        if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 1 <= layers <= top:
            raise ValueError(f"layers must be an int from 1 to {top}, got {layers!r}")
        if front not in ("plane", "model"):
            raise ValueError(f"front must be 'plane' or 'model', got {front!r}")
        try:
            ground = [float(v) for v in background]
        except (TypeError, ValueError):
            ground = []
        top32 = float(np.finfo(np.float32).max)        # (finite as the float32 the library takes)
        if len(ground) != 3 or not all(abs(v) <= top32 for v in ground):
            raise ValueError(f"background must be three finite numbers, got {background!r}")
        light = None
        if light_direction is not None:
            try:
                light = [float(v) for v in light_direction]
            except (TypeError, ValueError):
                light = []
            if len(light) != 3 or not all(abs(v) <= top32 for v in light):
                raise ValueError(f"light_direction must be None or three finite numbers, got {light_direction!r}")
            light = (C.c_float * 3)(*light)
        host = None
        if isinstance(alpha, torch.Tensor):
            if alpha.dtype != torch.float32 or alpha.dim() != 1:
                raise ValueError(f"alpha must be a number or float32 [T], got {alpha.dtype} {tuple(alpha.shape)}")
        else:
            if isinstance(alpha, (bool, np.bool_)) or not (isinstance(alpha, number) or isinstance(alpha, np.ndarray)):
                raise ValueError(f"alpha must be a number or an array [T], got {alpha!r}")
            host = np.asarray(alpha)
            if host.dtype.kind not in "fiu" or host.ndim > 1:
                raise ValueError(f"alpha must be a number or an array [T], got {host.dtype} {host.shape}")
            outside = int((~((host >= 0) & (host <= 1))).sum())       # (a NaN is outside)
            if outside:
                raise ValueError("alpha must lie in [0, 1]" + (f", got {alpha!r}" if host.ndim == 0 else
                                                              f": {outside} of {host.size} values do not"))
        self._pass_target("transparency_pass")
        T = self._pass_frame("transparency_pass")[1]
        if (host is not None and host.ndim == 1 and host.shape[0] != T) or (host is None and alpha.shape[0] != T):
            raise ValueError(f"transparency_pass: alpha holds {(alpha if host is None else host).shape[0]} triangles, "
                             f"the last frame drew {T}")
        tri, col, nrm, T, pos_of, (keys, trans, wins, zs) = self._peel_frame("transparency_pass")
        device = self.color_buffer.device
        if host is None:
            alpha_t = alpha.to(device).contiguous()
        elif host.ndim == 0:
            alpha_t = torch.full((T,), float(host), dtype=torch.float32, device=device)
        else:
            alpha_t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(device)
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        out = new((self.h, self.w, 3), dtype=torch.float32, device=device)
        ground3 = (C.c_float * 3)(*ground)
        n = int(layers)
        tail = (self.h, self.w, self.y0, self.y1)
        winner, z = self.winner_buffer, self.z_buffer
        for k in range(n):
            if k:
                self._launch_pass("crender_peel_next", (winner, z, tri, T, pos_of, self._P, nrm, keys, wins[k & 1], zs[k & 1]) +
                                  tail + (0,))
                winner, z = wins[k & 1], zs[k & 1]
            flags = (_capi.PEEL_FIRST if k == 0 else 0) | (_capi.PEEL_LAST if k == n - 1 else 0)
            self._launch_pass("crender_peel_blend", (winner, tri, T, pos_of, self._P, col, nrm, alpha_t if T else None, light,
                                                     self.color_buffer if k == 0 and front == "plane" else None, ground3,
                                                     trans, out) + tail + (flags,))
        return out

    def contour_edges(self, partners, static=None, borders=False):
        """uint8 [T] on the device: the edge mask of the LAST frame's view, ready for ``wire_pass(edges=...)``
        (``crender_wire_contours``, include/crender_wire.h).  Bit e of entry t is set if the edge of triangle t from
        corner e to corner (e + 1) % 3 is a contour — it lies between a triangle whose projection is wound one way and
        one wound the other: the line that bounds a smooth body, which changes with every pose — or is set in `static`,
        or, with `borders`, has no partner or more than one.  `partners` is the mesh's partner table, int32 [T, 3]
        (``wireframe.edge_partners``, made once per model), and `static` None or a uint8 [T] mask of edges drawn in
        every view (``wireframe.feature_edges``); both numpy arrays or device tensors in the caller's triangle order,
        with T that of the last frame, which, as for ``wire_pass``, started from cleared buffers and is not a swap
        chain's.  Two launches over the triangles on torch's current stream.

        The pass reads the last frame's triangles and the camera's projection, never a plane: it needs no winner plane,
        does not settle the frame (a frame rendered again after a bin overflow is drawn from the same triangles) and
        does not synchronise."""
        if self._pipeline:
            raise ValueError("contour_edges is not available on a swap chain (pipeline=True): per-slot passes are not implemented")
        tri, T = self._pass_frame("contour_edges")
        p = _device_array(self, partners, torch.int32, lambda s: len(s) == 2 and s[1] == 3,
                          "partners must be int32 [T, 3] (wireframe.edge_partners)")
        if p.shape[0] != T:
            raise ValueError(f"contour_edges: the partner table holds {p.shape[0]} triangles, the last frame drew {T}")
        if static is not None:
            static = _device_array(self, static, torch.uint8, lambda s: len(s) == 1, "static must be uint8 [T]")
            if static.shape[0] != T:
                raise ValueError(f"contour_edges: the static mask holds {static.shape[0]} triangles, the last frame drew {T}")
        facing = torch.empty(T, dtype=torch.int8, device=self.device)
        edges = torch.empty(T, dtype=torch.uint8, device=self.device)
        if T:
            pos_of = None if self._order is None else self._order[1]
            self._launch_pass("crender_wire_contours", (tri, T, pos_of, self._P, p, static, facing, edges, self.h, self.w,
                                                        _capi.WIRE_CONTOUR_BORDERS if borders else 0))
        return edges
