"""Bloom and tone mapping (``crender_bloom``, include/crender_bloom.h "Bloom"): a glow around what is brighter than a
threshold — the bright values blurred along the rows, then along the columns, and added to the source — and a curve that
brings the range back into 0 .. 255.  A post-process over any float32 image [H, W, 3] on the device.

``gaussian`` makes the table of weights; ``bloom`` runs the pass on a tensor; ``DevicePlanes.bloom`` (the fillers') and
``Renderer(bloom=...)`` run it on a filler's frame or on the tensor of the pass that ran last.  ``arguments`` and
``launch`` are what the three share."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _capi

MAX_RADIUS = _capi.BLOOM_MAX_RADIUS
KEYS = ("threshold", "radius", "weights", "intensity", "exposure", "tonemap", "white", "gamma", "clamp", "dtype", "flip_rows")

# What crender_bloom takes besides the planes; `weights` is a float32 array of radius + 1.
Call = namedtuple("Call", "threshold weights radius intensity exposure inv_white2 clamp flags dtype")


def gaussian(radius, sigma=None):
    """float32 [radius + 1]: exp(-k^2 / 2 sigma^2) for k = 0 .. radius in float64, sigma = radius / 3 by default, scaled
    so that w0 + 2 (w1 + ... + w_radius) is 1 in float64, then rounded."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be an int from 1 to {MAX_RADIUS}, got {radius!r}")
    sigma = radius / 3.0 if sigma is None else sigma
    if not _number(sigma) or not np.isfinite(sigma) or not sigma > 0:
        raise ValueError(f"sigma must be a finite number above 0, got {sigma!r}")
    k = np.arange(int(radius) + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def arguments(threshold=255.0, radius=8, weights=None, intensity=1.0, exposure=1.0, tonemap=None, white=float("inf"), gamma=1,
              clamp=None, dtype="float32", flip_rows=False):
    """The checked arguments of a call as a ``Call``; each bad one raises a ValueError that names it."""
    if not _number(threshold) or not threshold >= 0:
        raise ValueError(f"threshold must be a number, 0 or above, got {threshold!r}")
    if weights is None:
        weights = gaussian(radius)
    else:
        try:
            weights = np.ascontiguousarray(weights, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"weights must be a table of 2 to {MAX_RADIUS + 1} finite numbers, got {weights!r}") from None
        if weights.ndim != 1 or not 2 <= len(weights) <= MAX_RADIUS + 1 or not np.isfinite(weights).all():
            raise ValueError(f"weights must be a table of 2 to {MAX_RADIUS + 1} finite numbers, got {weights!r}")
    for name, v in (("intensity", intensity), ("exposure", exposure)):
        if not _number(v) or not abs(v) <= float(np.finfo(np.float32).max) or v < 0:        # (finite as a float32)
            raise ValueError(f"{name} must be a finite number, 0 or above, got {v!r}")
    if tonemap not in (None, "none", "reinhard"):
        raise ValueError(f"tonemap must be None, 'none' or 'reinhard', got {tonemap!r}")
    if not _number(white) or not white > 0:
        raise ValueError(f"white must be a number above 0 (inf: the plain operator), got {white!r}")
    if isinstance(gamma, bool) or gamma not in (1, 2):
        raise ValueError(f"gamma must be 1 or 2, got {gamma!r}")
    if dtype not in ("float32", "uint8"):
        raise ValueError(f"dtype must be 'float32' or 'uint8', got {dtype!r}")
    if clamp is None:
        clamp = 255.0 if dtype == "uint8" else float("inf")
    elif not _number(clamp) or clamp != clamp:
        raise ValueError(f"clamp must be None or a number, got {clamp!r}")
    with np.errstate(over="ignore", divide="ignore"):
        inv_white2 = float(np.float32(np.float64(1.0) / (np.float64(white) * np.float64(white))))
    flags = (_capi.BLOOM_U8 if dtype == "uint8" else 0) | (_capi.BLOOM_FLIP if flip_rows else 0) | \
        (_capi.BLOOM_REINHARD if tonemap == "reinhard" else 0) | (_capi.BLOOM_GAMMA2 if gamma == 2 else 0)
    return Call(float(threshold), weights, len(weights) - 1, float(intensity), float(exposure), inv_white2, float(clamp), flags,
                dtype)


def check_image(image, what="image"):
    if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() != 3 or image.shape[2] != 3 \
            or image.shape[0] < 1 or image.shape[1] < 1 or not image.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 [H, W, 3] device tensor, got "
                         f"{tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__}"
                         f"{' ' + str(image.dtype) if isinstance(image, torch.Tensor) else ''}")


def launch(lib, src, scratch, out, call, y0, y1, stream):
    """``crender_bloom`` of rows y0 .. y1 of `src` into `out`, on `stream`; `scratch` float32 like `src`."""
    H, W = int(src.shape[0]), int(src.shape[1])
    w = (C.c_float * len(call.weights))(*call.weights.tolist())
    _capi.check(lib.crender_bloom(src.data_ptr(), call.threshold, w, call.radius, call.intensity, call.exposure,
                                  call.inv_white2, call.clamp, scratch.data_ptr(), out.data_ptr(), H, W, y0, y1, call.flags,
                                  stream), "crender_bloom")


def bloom(image, **kw):
    """A NEW tensor [H, W, 3], float32 or uint8: `image` (a contiguous float32 [H, W, 3] device tensor, only read) with
    the glow of its bright pixels, tone mapped and clamped, on torch's current stream.  The keywords are
    ``DevicePlanes.bloom``'s but ``source``."""
    unknown = sorted(set(kw) - set(KEYS))
    if unknown:
        raise ValueError(f"bloom takes the keywords {', '.join(KEYS)}: {unknown} unknown")
    call = arguments(**kw)
    check_image(image)
    if not image.is_cuda:
        raise ValueError("image must be on the device: there is no CPU form of the pass")
    with torch.cuda.device(image.device):
        out = torch.empty(tuple(image.shape), dtype=getattr(torch, call.dtype), device=image.device)
        launch(_capi.load(), image, torch.empty_like(image), out, call, 0, int(image.shape[0]),
               C.c_void_p(torch.cuda.current_stream(image.device).cuda_stream))
    return out
