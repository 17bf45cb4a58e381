"""What the fillers that keep their framebuffers in HBM share (``AdvancedPixelBufferFiller``,
``EdgeOnlyPixelBufferFiller``): the three planes in the reference's initial state, and the HOST-VIEW
PROTOCOL that makes them look like the reference's own numpy buffers (.pyx:246-253).  Getters hand out
writable numpy views of PINNED host buffers, allocated once per plane, that stay valid and show every
later render: in-place changes are carried to the device before the next compositing render, and every
array handed out so far is refreshed at the end of a render.
  * ``_host_exposed``: the caller may have written into the views.  The next compositing render carries
    them to the device first (``_push_host_edits``); a frame that starts from cleared planes voids them
    instead (the filler stores ``_host_exposed = False``).
  * ``_host_fresh``: the views equal the planes.  Whatever writes the planes stores ``False``; a getter,
    or a render that refreshes the views, copies the handed-out planes back (``_refresh_mirrors``).
Only planes that have been handed out cross PCIe (one asynchronous copy each way per render); a filler
nobody asked a buffer of copies nothing.

A filler supplies ``device, h, w, y0, y1, _lib``, calls ``_allocate_planes`` when it has a GPU, and defines
  ``_ready_planes()``  make the planes usable on the current stream (create them, order the stream after
                       whatever renders into them elsewhere); no host synchronisation;
  ``_wait_planes()``   wait until the planes hold the finished frame; True if a frame was rendered again
                       meanwhile (the planes changed since the call began).
What needs the GPU or the library is in leaf methods of its own; the protocol around them only copies
tensors, so tests/test_host_views_cpu.py runs it on CPU tensors.
"""
import ctypes as C

import torch

from .. import _capi


class DevicePlanes:
    _bloom_scratch = None              # {(H, W): float32 [H, W, 3]}: bloom's row-blurred plane, made at the first call

    def __init__(self):
        self.z_buffer = self.color_buffer = self.normals_buffer = self.winner_buffer = None
        self._host = {}                # name -> numpy view handed out by a getter (of _host_pin[name])
        self._host_pin = {}            # name -> pinned host tensor behind the view
        self._host_fresh = False       # the views equal the device planes
        self._host_exposed = False     # a view was handed out and may have been edited

    # ------------------------------------------- leaves: the GPU and the library --
    def _allocate_planes(self, track_winner=False):
        """The planes in the state __cinit__ leaves (.pyx:65-67)."""
        with torch.cuda.device(self.device):
            self.z_buffer = torch.full((self.h, self.w), 1e6, dtype=torch.float32, device=self.device)
            self.color_buffer = torch.zeros((self.h, self.w, 3), dtype=torch.float32, device=self.device)
            self.normals_buffer = torch.zeros((self.h, self.w, 3), dtype=torch.float32, device=self.device)
            self.winner_buffer = torch.full((self.h, self.w), -1, dtype=torch.int32, device=self.device) if track_winner else None

    def _pinned_like(self, buf):
        with torch.cuda.device(self.device):
            return torch.empty(tuple(buf.shape), dtype=buf.dtype, pin_memory=True)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _win_ptr(self):
        return self.winner_buffer.data_ptr() if self.winner_buffer is not None else None

    def _clear_planes(self):
        with torch.cuda.device(self.device):
            _capi.check(self._lib.crender_clear(self.z_buffer.data_ptr(), self.color_buffer.data_ptr(),
                                                self.normals_buffer.data_ptr(), self._win_ptr(), self.h, self.w,
                                                self.y0, self.y1, self._stream()), "crender_clear")

    def _present_planes(self, flip_rows):
        out = torch.empty((self.h, self.w, 3), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.crender_present_u8(self.color_buffer.data_ptr(), out.data_ptr(), self.h, self.w,
                                                     1 if flip_rows else 0, self._stream()), "crender_present_u8")
        return out

    def _shade_planes(self, light):
        _capi.check(self._lib.crender_guro_illumination(
            self.color_buffer.data_ptr(), self.normals_buffer.data_ptr(), (C.c_float * 3)(*light),
            self.h, self.w, self.y0, self.y1, self._stream()), "crender_guro_illumination")

    def _resolve_planes(self, out, factor, light, flags, Y0, Y1):
        """crender_ssaa_resolve (include/crender_ssaa.h) of the colour plane into output rows Y0 .. Y1 of `out`."""
        with torch.cuda.device(self.device):
            _capi.check(self._lib.crender_ssaa_resolve(
                self.color_buffer.data_ptr(), None if light is None else self.normals_buffer.data_ptr(),
                None if light is None else (C.c_float * 3)(*light), self.h, self.w, factor, Y0, Y1,
                out.data_ptr(), flags, self._stream()), "crender_ssaa_resolve")

    def _bloom_planes(self, src, scratch, out, call, y0, y1):
        """crender_bloom (include/crender_bloom.h, "Bloom") of rows y0 .. y1 of `src` into `out`."""
        from .. import bloom
        with torch.cuda.device(self.device):
            bloom.launch(self._lib, src, scratch, out, call, y0, y1, self._stream())

    # ----------------------------------------------------------------- protocol --
    def _planes(self):
        return {"z": self.z_buffer, "color": self.color_buffer, "normals": self.normals_buffer}

    def _push_host_edits(self):
        """Carry in-place edits of handed-out numpy views back to the device."""
        self._ready_planes()
        if not self._host_exposed:
            return
        planes = self._planes()
        for name, pin in self._host_pin.items():
            planes[name].copy_(pin, non_blocking=True)        # (pinned: one DMA, stream-ordered)
        self._host_exposed = False

    def _refresh_mirrors(self, only=None):
        """Bring the handed-out arrays up to date with the device planes: one asynchronous copy per
        plane into its pinned buffer, issued BEFORE the wait so that one wait covers both (a frame
        that has to be redone — rare — is copied again)."""
        names = [n for n in self._host_pin if only is None or n in only]
        while True:
            self._ready_planes()
            planes = self._planes()
            for n in names:
                self._host_pin[n].copy_(planes[n], non_blocking=True)
            if not self._wait_planes():
                break
        if only is None:
            self._host_fresh = True
            # The arrays the caller holds show the planes again — and are the caller's to write into from here on,
            # getter call or not: the next compositing render carries them back first.  (While only a getter call
            # raised this flag, an edit made after a render into arrays handed out before it never reached the device.)
            if self._host:
                self._host_exposed = True

    def _mirror(self, name):
        if not self._host_fresh:
            self._refresh_mirrors()
        if name not in self._host:
            self._host_pin[name] = self._pinned_like(self._planes()[name])
            self._host[name] = self._host_pin[name].numpy()
            self._refresh_mirrors(only=(name,))
        self._host_exposed = True
        return self._host[name]

    def get_normals_buffer(self):
        return self._mirror("normals")

    def get_color_buffer(self):
        return self._mirror("color")

    def get_z_buffer(self):
        return self._mirror("z")

    # --------------------------------------------------------------- extensions --
    def get_z_tensor(self):
        self._ready_planes()
        return self.z_buffer

    def get_color_tensor(self):
        self._ready_planes()
        return self.color_buffer

    def get_normals_tensor(self):
        self._ready_planes()
        return self.normals_buffer

    def clear(self):
        """Back to the state __cinit__ leaves (.pyx:65-67): colour 0, z 1e6, normals 0."""
        self._ready_planes()
        self._clear_planes()
        self._host_fresh = False
        self._host_exposed = False

    def present_u8(self, flip_rows=True):
        """uint8 [H, W, 3] device tensor of the colour plane, rows flipped: what run.py:26 writes to disk."""
        self.get_color_tensor()        # (what the filler does before it hands the plane out: it must be complete)
        self._push_host_edits()
        return self._present_planes(flip_rows)

    def resolve(self, factor, light_direction=None, dtype="float32", flip_rows=False):
        """Supersampled anti-aliasing: a NEW device tensor [h / factor, w / factor, 3] whose pixels are the means
        of the factor x factor blocks of the colour plane (``crender_ssaa_resolve``, include/crender_ssaa.h: the
        samples of a block summed in row-major order, one float32 division).  With `light_direction` (the
        illumination object's own flipped, normalised vector, as ``texture_pass`` and ``set_fused_illumination``
        take it) every sample is shaded as it is read — the bits of ``shade_guro`` followed by the plain
        resolve, without that pass over the supersampled planes.  `dtype` "uint8" stores
        ``present_u8``'s cast of the mean and `flip_rows` stores the rows bottom up:
        ``resolve(s, dtype="uint8", flip_rows=True)`` is the image run.py:26 writes to disk.

        Edits made in the numpy views handed out so far are carried to the device first, and the frame is
        settled after the launch (one stream synchronisation per call, as every getter and ``texture_pass``
        pay): a frame whose bin lists overflowed is rendered again, and resolved again into the same tensor.
        A filler with a ``row_strip`` resolves its rows (both ends multiples of `factor`) and leaves the other
        rows of the result zero.  The planes are only read: the views stay as fresh or as stale as they were."""
        if isinstance(factor, bool) or not isinstance(factor, int) or not 1 <= factor <= _capi.SSAA_MAX:
            raise ValueError(f"factor must be an int from 1 to {_capi.SSAA_MAX}, got {factor!r}")
        if dtype not in ("float32", "uint8"):
            raise ValueError(f"dtype must be 'float32' or 'uint8', got {dtype!r}")
        self._push_host_edits()        # (first of all: a filler may create its planes here)
        if self.h % factor or self.w % factor:
            raise ValueError(f"the frame {self.h} x {self.w} is not a multiple of factor={factor} in both directions")
        if self.y0 % factor or self.y1 % factor:
            raise ValueError(f"the row strip ({self.y0}, {self.y1}) must start and end on multiples of factor={factor}")
        light = None if light_direction is None else [float(v) for v in light_direction]
        flags = (_capi.SSAA_U8 if dtype == "uint8" else 0) | (_capi.SSAA_FLIP if flip_rows else 0)
        new = torch.empty if (self.y0, self.y1) == (0, self.h) else torch.zeros
        out = new((self.h // factor, self.w // factor, 3), dtype=getattr(torch, dtype), device=self.color_buffer.device)
        while True:
            self._resolve_planes(out, factor, light, flags, self.y0 // factor, self.y1 // factor)
            if not self._wait_planes():
                break
            self._ready_planes()       # (a frame was rendered again: the same planes, settled now)
        return out

    def bloom(self, threshold=255.0, radius=8, weights=None, intensity=1.0, exposure=1.0, tonemap=None, white=float("inf"),
              gamma=1, clamp=None, dtype="float32", flip_rows=False, source=None):
        """Bloom and tone mapping (``crender_bloom``, include/crender_bloom.h "Bloom"): a NEW device tensor [H, W, 3] that
        holds the image with a glow around its bright pixels.  A pixel whose largest channel m exceeds `threshold` is
        bright by (m - threshold) / m of its colour; the bright values are blurred with `weights` (a table of radius + 1
        numbers by distance; None: ``bloom.gaussian(radius)``; an explicit table fixes radius = len - 1, at most 32) along
        the rows and then along the columns, and `intensity` times the glow is added.  A pixel no glow reaches keeps its
        bits.  Then, only if asked for: `exposure` scales, `tonemap` "reinhard" maps a = v / 255 to
        a (1 + a / white^2) / (1 + a), `gamma` 2 takes the square root; `clamp` cuts from above.  `dtype` "uint8"
        stores ``present_u8``'s cast (clamped at 255 unless `clamp` says otherwise) and `flip_rows` stores the rows
        bottom up: ``bloom(dtype="uint8", flip_rows=True)`` is the PNG's bytes.

        Without `source` the image is the filler's colour plane, completed as ``present_u8`` completes it (edits made
        in the numpy views are carried up first; a frame whose bin lists overflowed is rendered again and bloomed
        again), over the filler's rows; the other rows of the result are zero.  The planes are only read: the views
        stay as fresh or as stale as they were.  With `source`, a contiguous float32 [H', W', 3] tensor on the filler's
        device, of any size — what ``edge_aa``, ``depth_of_field``, ``transparency_pass`` or ``resolve`` returned —
        the pass runs over all of its rows.  On torch's current stream; the scratch plane is kept per shape."""
        from .. import bloom
        call = bloom.arguments(threshold, radius, weights, intensity, exposure, tonemap, white, gamma, clamp, dtype, flip_rows)
        if source is None:
            self.get_color_tensor()    # (what the filler does before it hands the plane out: it must be complete)
            self._push_host_edits()
            src, y0, y1 = self.color_buffer, self.y0, self.y1
        else:
            bloom.check_image(source, "source")
            want = torch.device(self.device)
            if source.device.type != want.type or (want.index is not None and source.device.index != want.index):
                raise ValueError(f"source must be on the filler's device {want}, got {source.device}")
            src, y0, y1 = source, 0, int(source.shape[0])
        H, W = int(src.shape[0]), int(src.shape[1])
        if self._bloom_scratch is None:
            self._bloom_scratch = {}
        scratch = self._bloom_scratch.get((H, W))
        if scratch is None:
            scratch = self._bloom_scratch[(H, W)] = torch.empty((H, W, 3), dtype=torch.float32, device=src.device)
        new = torch.empty if (y0, y1) == (0, H) else torch.zeros
        out = new((H, W, 3), dtype=getattr(torch, call.dtype), device=src.device)
        while True:
            self._bloom_planes(src, scratch, out, call, y0, y1)
            if source is not None or not self._wait_planes():
                break
            self._ready_planes()       # (a frame was rendered again: the same planes, settled now)
        return out

    def shade_guro(self, light):
        """``GuroIllumination.draw_illumination`` over rows y0 … y1 of the planes; `light`: that class's vector, as floats."""
        self._shade_planes(light)
        self._host_fresh = False
