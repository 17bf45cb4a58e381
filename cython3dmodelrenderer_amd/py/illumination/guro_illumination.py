"""The py ``GuroIllumination`` (crender/py/illumination/guro_illumination.py): the package's float32
shade (same light vector, same factor) applied to the uint8 colour Buffer,
``(colour.astype(float32) * shade).astype(uint8)``.

The reference reads the normals as ``n_buffer[[...]]``, which numpy >= 1.23 rejects (IndexError); what
it meant, ``n_buffer[...]``, is what is computed here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ...illumination import GuroIllumination as _FloatGuro


class GuroIllumination(_FloatGuro):
    def draw_illumination(self, color_buffer, n_buffer):
        normals = n_buffer[...]
        cos = np.sum(normals * self.light_direction, axis=-1, keepdims=True)
        factor = np.clip(cos / (np.linalg.norm(normals, axis=-1, keepdims=True) + 1e-6), 0, 1)
        shaded = color_buffer[...].astype(np.float32) * factor
        with np.errstate(invalid="ignore"):               # (a NaN factor: numpy's cast gives 0)
            color_buffer[...] = shaded.astype(np.uint8)

    def draw_illumination_device(self, color, normals):
        """The same on device tensors: ``color`` uint8 [H, W, 3], ``normals`` float32 [H, W, 3]
        (crender_py_guro), in place on the current stream."""
        import torch
        from ... import _capi
        lib = _capi.load()
        if color.dtype != torch.uint8 or normals.dtype != torch.float32 or color.dim() != 3 or \
                tuple(color.shape) != tuple(normals.shape) or color.shape[2] != 3 or \
                not color.is_contiguous() or not normals.is_contiguous():
            raise ValueError("draw_illumination_device takes contiguous uint8 and float32 [H, W, 3] tensors")
        h, w = int(color.shape[0]), int(color.shape[1])
        with torch.cuda.device(color.device):
            stream = C.c_void_p(torch.cuda.current_stream(color.device).cuda_stream)
            _capi.check(lib.crender_py_guro(color.data_ptr(), normals.data_ptr(),
                                            (C.c_float * 3)(*self.light_direction.tolist()), h, w, stream),
                        "crender_py_guro")
