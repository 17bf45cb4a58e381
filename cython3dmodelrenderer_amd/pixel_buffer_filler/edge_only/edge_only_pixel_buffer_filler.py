"""Wireframe filler: the reference's ``EdgeOnlyPixelBufferFiller``
(crender/py/pixel_buffer_filler/edge_only/edge_only_pixel_buffer_filler.py:8-33), with a whole-mesh
``render_model`` on the GPU.

    EdgeOnlyPixelBufferFiller(line_drawer, line_color, draw_edges=True, force_triangle_colors=False,
                              *, h=None, w=None, device=None)

``compute_triangle_statistics`` is the reference's per-triangle method on the host: it calls the
given ``line_drawer`` and writes into any object with ``set_pixel(x, y, value)``.

``render_model(model)`` / ``render_arrays(tri, col)`` draw every triangle of a mesh, in index order,
onto a float32 colour plane [h][w][3] in HBM (csrc/wireframe.hip, include/crender_wire.h), bit for
bit what ``compute_triangle_statistics`` leaves when called on each triangle in turn with
``LineBresenham``.  The filler then behaves like ``AdvancedPixelBufferFiller`` towards its callers
(``Renderer``, the illuminations): the same three planes, initial state (colour 0, z 1e6, normals
0), getters of writable numpy views whose in-place edits are carried back before the next
compositing draw, device tensors, ``clear``, ``present_u8``: the code of both is
``.._device_planes.DevicePlanes``.  The z and normal planes are never drawn into.  The device path
needs ``h`` and ``w`` and the ``LineBresenham`` line (another ``draw_line`` raises TypeError: there is
no device form of it).

Domain: the GPU path is exact for vertex x / y with ``|c| < 2**30``.  Any other x / y (NaN, inf,
huge) raises ValueError before anything is drawn — the buffers keep their contents — where the
reference raises after drawing the triangles before it (NaN, inf) or loops for ages (huge).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ... import _capi
from .._device_planes import DevicePlanes
from .line_drawer import LineBresenham, LineDrawer

_MAX_ORDERED_T = 1 << 30     # per-triangle colours: a uint32 key 3 i + e + 1 per pixel


def _as_device(a, name, device, cast):
    """[T, 3, 3] contiguous float32 tensor on `device` from a numpy array or a torch tensor.  `cast`:
    convert other dtypes as numpy's assignment into a float32 buffer does (colours); otherwise
    float32 is required (vertex coordinates: ``int()`` of a float64 is not ``int()`` of its float32)."""
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.float32 and not cast:
            raise ValueError(f"{name} must be float32, got {a.dtype}")
        t = a.to(device=device, dtype=torch.float32).contiguous()
    else:
        arr = np.asarray(a)
        if arr.dtype != np.float32:
            if not cast:
                raise ValueError(f"{name} must be float32, got {arr.dtype}")
            arr = np.asarray(arr, dtype=np.float32)
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    if t.dim() != 3 or t.shape[1] != 3 or t.shape[2] != 3:
        raise ValueError(f"{name} must have shape [T, 3, 3], got {tuple(t.shape)}")
    return t


class EdgeOnlyPixelBufferFiller(DevicePlanes):
    def __init__(self, line_drawer: LineDrawer, line_color, draw_edges=True, force_triangle_colors=False,
                 *, h=None, w=None, device=None):
        super().__init__()             # the planes (None until _ensure_device) and the host-view state
        self.line_drawer = line_drawer
        self.line_color = line_color
        self.draw_edges = draw_edges
        self.force_triangle_colors = force_triangle_colors
        self.h = None if h is None else int(h)
        self.w = None if w is None else int(w)
        self.y0, self.y1 = 0, self.h          # (the whole frame: what the illuminations' device forms read)
        self.device = torch.device(device if device is not None else "cuda:0")
        # device state, made at the first draw or getter call
        self._lib = None
        self._key = None               # uint32 key plane of per-triangle colours (zero between draws)
        self._status = None            # device int32: the draw's domain flag
        self._status_host = None       # pinned copy of it
        self._fused_light = None

    # ------------------------------------------------------------- reference API --
    def compute_triangle_statistics(self, triangle, colors, normals, color_buffer, z_buffer, n_buffer):
        """One triangle on the host, through ``self.line_drawer`` (reference: :16-33)."""
        p = [[int(triangle[k][0]), int(triangle[k][1])] for k in range(3)]

        def colour(k):
            return colors[k] if self.force_triangle_colors else self.line_color

        if self.draw_edges:
            for k in range(3):
                self.line_drawer.draw_line(p[k], p[(k + 1) % 3], color_buffer, colour(k))
        else:
            for k in range(3):
                color_buffer.set_pixel(*p[k], colour(k))

    def get_size(self):
        return self.h, self.w

    # --------------------------------------------------------------- device path --
    def _check_device_path(self):
        if type(self.line_drawer).draw_line is not LineBresenham.draw_line:
            raise TypeError(f"render_model draws LineBresenham lines on the GPU; "
                            f"{type(self.line_drawer).__name__}.draw_line has no device form "
                            "(use compute_triangle_statistics)")
        if self.h is None or self.w is None:
            raise ValueError("render_model needs the frame size: EdgeOnlyPixelBufferFiller(..., h=H, w=W)")

    def _ensure_device(self):
        if self.color_buffer is not None:
            return
        if self.h is None or self.w is None:
            raise ValueError("the device buffers need the frame size: EdgeOnlyPixelBufferFiller(..., h=H, w=W)")
        lib = _capi.load()                             # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise _capi.CrenderError("EdgeOnlyPixelBufferFiller.render_model needs a ROCm GPU (no CPU fallback)")
        if lib.crender_wire_key_bytes(self.h, self.w) == 0:
            raise ValueError(f"bad frame size for the wireframe filler: h={self.h} w={self.w}")
        self._allocate_planes()
        with torch.cuda.device(self.device):
            self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._status_host = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        self._lib = lib

    _ready_planes = _ensure_device     # (DevicePlanes' hooks)

    def _wait_planes(self):
        torch.cuda.current_stream(self.device).synchronize()
        return False

    def render_model(self, model, refresh=False, clear=False, refresh_views=True):
        """Draw the wireframe of ``model`` (a ``Model``, a ``DeviceModel``, anything with
        ``_vertices_by_triangles`` and ``_colors_by_triangles``) on top of the current buffers, its
        triangles in index order.  ``clear=True`` starts from the initial state in the same call.
        ``refresh_views=False`` leaves the numpy views handed out earlier stale until the next getter
        call.  (``refresh``: accepted for the shaded filler's signature; nothing is cached.)"""
        self.render_arrays(model._vertices_by_triangles, getattr(model, "_colors_by_triangles", None),
                           clear=clear, refresh_views=refresh_views)

    render = render_model

    def render_arrays(self, tri, col=None, clear=False, refresh_views=True):
        """``render_model`` on explicit [T, 3, 3] arrays (numpy or torch, any device): vertices
        (float32; x and y are used), and the colours per corner that ``force_triangle_colors`` takes."""
        self._check_device_path()
        if self.force_triangle_colors and col is None:
            raise ValueError("force_triangle_colors needs the triangles' colours (the model has none)")
        self._ensure_device()
        tri = _as_device(tri, "vertices", self.device, cast=False)
        T = int(tri.shape[0])
        flags = (0 if self.draw_edges else _capi.WIRE_DOTS) | (_capi.WIRE_CLEAR if clear else 0)
        colp = keyp = None
        if self.force_triangle_colors:
            if T >= _MAX_ORDERED_T:
                raise ValueError(f"force_triangle_colors draws fewer than 2**30 triangles at once, got {T}")
            col = _as_device(col, "colours", self.device, cast=True)
            if col.shape[0] != T:
                raise ValueError("vertex and colour arrays must have the same shape")
            if self._key is None:
                with torch.cuda.device(self.device):
                    self._key = torch.zeros(self.h * self.w, dtype=torch.int32, device=self.device)
            flags |= _capi.WIRE_FORCE_COLORS
            colp, keyp = col.data_ptr(), self._key.data_ptr()
        # the cast numpy's assignment into a float32 buffer applies (buffer.py:69)
        line = np.broadcast_to(np.asarray(self.line_color, np.float32), (3,))
        if not clear:
            self._push_host_edits()
        with torch.cuda.device(self.device):
            stream = self._stream()
            _capi.check(self._lib.crender_wire_draw(
                tri.data_ptr(), colp, T, (C.c_float * 3)(*line.tolist()), self.z_buffer.data_ptr(),
                self.color_buffer.data_ptr(), self.normals_buffer.data_ptr(), keyp, self.h, self.w, flags,
                self._status.data_ptr(), stream), "crender_wire_draw")
            # the one synchronisation of a draw: the domain flag (inputs stay alive until it returns)
            self._status_host.copy_(self._status, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        if int(self._status_host[0]):
            raise ValueError("vertex x / y out of the wireframe filler's domain (NaN, inf or |c| >= 2**30): "
                             "nothing was drawn")
        if clear:
            self._host_exposed = False         # (edits of the views are void: the frame started afresh)
        self._host_fresh = False
        if clear and self._fused_light is not None:
            with torch.cuda.device(self.device):
                self.shade_guro(self._fused_light)
        if self._host and refresh_views:
            self._refresh_mirrors()

    def set_fused_illumination(self, light_direction=None):
        """``GuroIllumination.fuse_into``: shade every frame drawn with ``clear=True`` before it is handed
        out — the same kernel as the unfused device form (crender_guro_illumination), so the same bits.
        ``None`` switches it off."""
        self._fused_light = None if light_direction is None else tuple(float(v) for v in light_direction)

    def synchronize(self):
        if self.color_buffer is not None:
            torch.cuda.current_stream(self.device).synchronize()
