"""Temporal anti-aliasing, the part that is plain array arithmetic: the sub-pixel offsets of a frame cycle and the view
shear that moves a frame's image by such an offset.  (The resolve against the history is
``AdvancedPixelBufferFiller.temporal_resolve``, include/crender_taa.h; ``Renderer(temporal_aa=...)`` runs the two.)

The offset is a SHEAR of the vertices, ``x' = x + z * kx``, ``y' = y + z * ky``, not an entry of the projection matrix: the
projection divides by z, so the shear moves every projected point by the same ``kx * P[0] * w / 2`` pixels, the frame's
resident triangles are the sheared ones, and every pass that projects them again stays consistent with the frame it
sees (several refuse a matrix with entries 8 or 9 set).  The numpy form of ``sheared`` is the rule; the torch form makes
the same two float32 operations per coordinate."""
import numpy as np


def _radical_inverse(i, base):
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def jitter_offsets(n):
    """float64 [n, 2]: the first `n` points of the Halton (2, 3) sequence, index 1 .. n, each minus 1/2: pairs (jx, jy)
    of pixels in [-1/2, 1/2)."""
    n = int(n)
    if n < 0:
        raise ValueError(f"n must be 0 or above, got {n}")
    return np.array([[_radical_inverse(i, 2) - 0.5, _radical_inverse(i, 3) - 0.5] for i in range(1, n + 1)],
                    dtype=np.float64).reshape(n, 2)


def view_shear(P, h, w, jx, jy):
    """(kx, ky), float32: the shear that moves the image of a frame `h` x `w` under the projection `P` (the filler's
    matrix, 4 x 4 or its 16 entries) by (jx, jy) pixels.  Each is one float64 quotient, rounded once."""
    P16 = np.asarray(P, dtype=np.float32).reshape(16)
    xs, ys = np.float32(w / 2.0), np.float32(h / 2.0)
    return (np.float32(float(jx) / (float(xs) * float(P16[0]))), np.float32(float(jy) / (float(ys) * float(P16[5]))))


def sheared(vertices, kx, ky):
    """A new [T, 3, 3] float32 array of the kind of `vertices` (numpy in, numpy out; a tensor in, a tensor on its device
    out) with ``x' = x + z * kx`` and ``y' = y + z * ky``, each one float32 product and one float32 sum; z is unchanged."""
    kx, ky = np.float32(kx), np.float32(ky)
    if isinstance(vertices, np.ndarray):
        if vertices.dtype != np.float32 or vertices.ndim != 3 or vertices.shape[1:] != (3, 3):
            raise ValueError(f"vertices must be float32 [T, 3, 3], got {vertices.dtype} {vertices.shape}")
        out = np.array(vertices, dtype=np.float32, order="C", copy=True)
        z = out[..., 2]
        out[..., 0] = out[..., 0] + z * kx
        out[..., 1] = out[..., 1] + z * ky
        return out
    import torch
    if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32 or vertices.dim() != 3 \
            or tuple(vertices.shape[1:]) != (3, 3):
        raise ValueError("vertices must be a float32 [T, 3, 3] numpy array or tensor, got "
                         f"{getattr(vertices, 'dtype', type(vertices).__name__)} {tuple(getattr(vertices, 'shape', ()))}")
    out = vertices.detach().clone(memory_format=torch.contiguous_format)
    z = out[..., 2]
    # (the product is a tensor of its own before the sum: two roundings, as in numpy; a float32 scalar is exact in Python's float)
    out[..., 0] = out[..., 0] + z * float(kx)
    out[..., 1] = out[..., 1] + z * float(ky)
    return out


class JitteredModel:
    """What a filler reads off a model, with the vertices of `model` sheared by (kx, ky) and its two other arrays as they
    are: the stand-in that ``Renderer(temporal_aa=...)`` draws."""

    def __init__(self, model, kx, ky):
        self._vertices_by_triangles = sheared(model._vertices_by_triangles, kx, ky)
        self._colors_by_triangles = model._colors_by_triangles
        self._normals_by_triangles = model._normals_by_triangles
