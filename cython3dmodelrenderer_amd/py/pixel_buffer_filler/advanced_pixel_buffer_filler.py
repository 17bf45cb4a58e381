"""The numpy filler of the reference's crender/py
(pixel_buffer_filler/advanced_pixel_buffer_filler.py:13-240) on ``Buffer`` planes: colour uint8, z
float32 and normals float32.

``compute_triangle_statistics`` draws one triangle on the host, with numpy, in the reference's
arithmetic (include/crender_py.h states it step by step): float64 barycentric numerators over float32
denominators, the depth and the attributes through ``np.dot`` (BLAS), a pixel kept iff
``0 <= z <= 1`` and ``z`` is below the stored float32, colours truncated to uint8.

``draw_sequence`` draws a whole ordered sequence of triangles onto the three Buffers on the GPU
(csrc/pyfill.hip, include/crender_py.h): bit for bit what calling ``compute_triangle_statistics`` on
each triangle in turn leaves.  Domain: finite inputs, vertex z != 0, T < 2**30, h and w at most
2**15; anything else raises ValueError before anything is drawn.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ..data_structures import Buffer

MAX_SIDE = 1 << 15


class AdvancedPixelBufferFiller:
    def __init__(self, h, w, fov=90.0, z_near=0.1, z_far=1000, device=None):
        self._h = h
        self._w = w
        self._fov = fov
        self._f = 1 / np.tan(self._fov / 2 / 180 * np.pi)
        self._z_near = z_near
        self._z_far = z_far
        self._a = h / w
        q = z_far / (z_far - z_near)
        # the float32 entries of the reference's projection matrix (:28-35); the others are 0 or 1
        self._proj = np.array([self._f / self._a, self._f, q, -z_near * q], dtype=np.float32)
        self._device = device
        self._dev = None

    def get_size(self):
        return self._h, self._w

    # ------------------------------------------------------------------ host --
    def _project(self, tri):
        P00, P11, P22, P32 = self._proj
        x, y, z = tri[:, 0], tri[:, 1], tri[:, 2]
        with np.errstate(all="ignore"):
            px = (x * P00 / z + np.float32(1)) * np.float32(self._w / 2)
            py = (y * P11 / z + np.float32(1)) * np.float32(self._h / 2)
            pz = (z * P22 + P32) / z
        return px, py, pz

    def compute_triangle_statistics(self, triangle, colors, normals, color_buffer: Buffer, z_buffer: Buffer,
                                    n_buffer: Buffer):
        assert color_buffer.get_size() == z_buffer.get_size() == n_buffer.get_size() == (self._h, self._w), \
            "Buffers' spatial dimensions must be the same"
        tri = np.asarray(triangle, np.float32)
        nrm = np.asarray(normals, np.float32)
        with np.errstate(all="ignore"):
            # degenerate in raw x / y: the float32 2-D cross
            e1, e2 = tri[1, :2] - tri[0, :2], tri[2, :2] - tri[0, :2]
            if e1[0] * e2[1] - e1[1] * e2[0] == 0:
                return
            # back-facing: the float64 dot of [0, 0, 1] with the float32 mean normal
            mean = ((nrm[0] + nrm[1]) + nrm[2]) / np.float32(3)
            if np.float64(0) * mean[0] + np.float64(0) * mean[1] + np.float64(mean[2]) >= 0:
                return
            px, py, pz = self._project(tri)
            xl, xr, yb, yt = (np.ceil(np.array([px.min(), px.max(), py.min(), py.max()], np.float32))
                              .astype(np.int32))
        xl, xr = np.clip([xl, xr], 0, self._w)
        yb, yt = np.clip([yb, yt], 0, self._h)
        ys, xs = np.mgrid[yb:yt, xl:xr]
        xs, ys = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
        with np.errstate(all="ignore"):
            lam = []
            for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                ax, ay = px[j] - px[k], py[j] - py[k]                          # float32
                den = ax * (py[i] - py[k]) - ay * (px[i] - px[k])            # float32
                num = ax * (ys - np.float64(py[k])) - ay * (xs - np.float64(px[k]))  # float64
                lam.append(num / np.float64(den))
            bar = np.stack(lam, axis=-1)
            inside = (bar >= 0).all(axis=-1)
            bar, xs, ys = bar[inside], xs[inside].astype(np.int64), ys[inside].astype(np.int64)
            if len(bar) == 0:
                return
            z = np.dot(bar, pz.astype(np.float64).reshape(3, 1))[:, 0]     # (the reference's [n,3] @ [3,1])
            keep = (z >= 0) & (z <= 1)
            bar, xs, ys, z = bar[keep], xs[keep], ys[keep], z[keep]
            keep = z < z_buffer[ys, xs][:, 0]
            bar, xs, ys, z = bar[keep], xs[keep], ys[keep], z[keep]
            z_buffer[ys, xs] = z[:, None]
            if len(bar) == 0:
                return
            color_buffer[ys, xs] = np.dot(bar, np.asarray(colors).astype(np.float64))
            n_buffer[ys, xs] = np.dot(bar, nrm.astype(np.float64))

    # ---------------------------------------------------------------- device --
    def _ensure_device(self):
        if self._dev is not None:
            return self._dev
        import torch
        from ... import _capi
        lib = _capi.load()                              # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise _capi.CrenderError("AdvancedPixelBufferFiller.draw_sequence needs a ROCm GPU (no CPU fallback)")
        device = torch.device(self._device if self._device is not None else "cuda:0")
        self._dev = (lib, device, torch.zeros(1, dtype=torch.int32, device=device))
        return self._dev

    def draw_sequence(self, tri, col, nrm, color_buffer: Buffer, z_buffer: Buffer, n_buffer: Buffer,
                      clear=False, light=None):
        """Draw the triangles ``tri`` with colours ``col`` and vertex normals ``nrm`` ([T, 3, 3] each) in
        array order onto the three Buffers, on the GPU.  ``clear=True`` starts from the Renderer's initial
        buffers instead of their contents.  ``light``: the normalised, negated light direction of a py
        ``GuroIllumination`` to apply to the colour plane after the draw, on the device.

        Input contract: vertices and normals float32 (the culls compute in the arrays' own dtype, so a
        float64 array would be another computation); colours of any real dtype whose values float32 holds
        exactly (the model's float32 colours, the integers 0..255 of the random and white ones), which
        the draw widens to float64 as numpy does.  Anything else raises ValueError, as do NaN and inf."""
        import torch
        from ... import _capi
        lib, device, status = self._ensure_device()
        h, w = self._h, self._w
        assert color_buffer.get_size() == z_buffer.get_size() == n_buffer.get_size() == (h, w), \
            "Buffers' spatial dimensions must be the same"
        arrays = []
        for name, a in (("vertices", tri), ("colours", col), ("normals", nrm)):
            a = np.asarray(a)
            if a.ndim != 3 or a.shape[1:] != (3, 3):
                raise ValueError(f"{name} must have shape [T, 3, 3], got {a.shape}")
            if name != "colours" and a.dtype != np.float32:
                raise ValueError(f"{name} must be float32, got {a.dtype}")
            if name == "colours":
                if a.dtype.kind not in "biuf":
                    raise ValueError(f"colours must be real numbers, got {a.dtype}")
                held = a.astype(np.float32)
                with np.errstate(invalid="ignore"):
                    exact = np.array_equal(held.astype(a.dtype), a)
                if not exact and np.all(np.isfinite(a)):
                    raise ValueError(f"{a.dtype} colours that float32 does not hold exactly: draw float32 ones")
                a = held
            if name != "vertices" and not np.all(np.isfinite(a)):
                raise ValueError(f"{name} out of the numpy filler's domain (NaN or inf): nothing was drawn")
            arrays.append(a)
        T = arrays[0].shape[0]
        if any(a.shape[0] != T for a in arrays):
            raise ValueError("vertex, colour and normal arrays must have the same length")
        scratch_bytes = lib.crender_py_scratch_bytes(h, w, T)
        if scratch_bytes == 0:
            raise ValueError(f"out of the numpy filler's domain: h={h} w={w} T={T} (h, w <= 2**15, T < 2**30)")
        planes = [z_buffer.get_image(), color_buffer.get_image(), n_buffer.get_image()]
        for p, dt, d in zip(planes, (np.float32, np.uint8, np.float32), (1, 3, 3)):
            if p.dtype != dt or p.shape != (h, w, d):
                raise ValueError(f"the draw needs the py Renderer's planes; got {p.dtype} {p.shape}")
        with torch.cuda.device(device):
            d_tri, d_col, d_nrm = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays)
            d_z, d_c, d_n = (torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in planes)
            scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            _capi.check(lib.crender_py_draw(
                d_tri.data_ptr(), d_col.data_ptr(), d_nrm.data_ptr(), T, (C.c_float * 4)(*self._proj.tolist()),
                d_z.data_ptr(), d_c.data_ptr(), d_n.data_ptr(), h, w, _capi.PY_CLEAR if clear else 0,
                scratch.data_ptr(), status.data_ptr(), stream), "crender_py_draw")
            if int(status.item()):                      # (synchronises the stream)
                raise ValueError("vertices out of the numpy filler's domain (NaN, inf or z == 0): nothing was drawn")
            if light is not None:
                _capi.check(lib.crender_py_guro(d_c.data_ptr(), d_n.data_ptr(),
                                                (C.c_float * 3)(*[float(v) for v in light]), h, w, stream),
                            "crender_py_guro")
            for p, d in zip(planes, (d_z, d_c, d_n)):
                p[...] = d.cpu().numpy()


__all__ = ["AdvancedPixelBufferFiller"]
