"""What a caller of ``AdvancedPixelBufferFiller.depth_of_field`` needs beside the pass: the view depth a value of the z
plane stands for, by the statement the kernel itself uses (include/crender_dof.h, "Depth of field"), so that the focus
can be put on what a pixel shows::

    z = filler.get_z_tensor()
    image = filler.depth_of_field(focus=view_depth(filler._P, z[y, x]), aperture=6.0)
"""
import numpy as np


def view_depth(P, z):
    """The view depth ``zv = P14 / (z - P10)`` of the z-plane value(s) `z` under the projection matrix `P` (4 x 4, or its
    16 floats in row order: ``filler._P``): one float32 subtraction and one float32 division, the kernel's own.  `z` may
    be a number or a numpy array (a float32 scalar or array comes back) or a torch tensor (a float32 tensor on its
    device comes back).  The background's z (1e6) gives a small negative number, not a depth: ask only about covered
    pixels."""
    P16 = np.asarray(P, dtype=np.float32).reshape(16)
    p10, p14 = P16[10], P16[14]
    try:
        import torch
    except ImportError:                # (numpy callers need no torch)
        torch = None
    if torch is not None and isinstance(z, torch.Tensor):
        below = z.to(torch.float32) - float(p10)
        return torch.full_like(below, float(p14)) / below      # (tensor by tensor: a number by a tensor multiplies a reciprocal)
    with np.errstate(all="ignore"):
        return p14 / (np.asarray(z, dtype=np.float32) - p10)
