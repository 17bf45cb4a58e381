"""The light's frame for ``AdvancedPixelBufferFiller.shadow_pass``: upload-time plumbing in numpy or torch, no kernel.

A shadow map here is an ordinary frame of a second filler, drawn from the light.  That filler looks down +z from
the origin like the camera's, so the model is carried into the light's frame first: ``look_at`` gives the rigid
motion, ``light_arrays`` applies it to a model's vertices and normals (the normals decide the light frame's
back-face test).  The moved vertices are also what ``bind_shadow_map`` takes."""
import numpy as np


def look_at(position, target, up=(0, -1, 0)):
    """(R float32 [3, 3], t float32 [3]) of a light at `position` that looks at `target`: a point p of the model
    has the light-frame coordinates R @ p + t.  The rows of R are the frame's right, down and forward axes (image
    y grows downwards, so the default `up` (0, -1, 0) is the direction of decreasing image rows), and
    t = -R @ position."""
    position, target, up = (np.asarray(v, np.float64).reshape(3) for v in (position, target, up))
    forward = target - position
    n = np.linalg.norm(forward)
    if not n > 0:
        raise ValueError("look_at: position and target coincide")
    forward = forward / n
    right = np.cross(forward, up)
    n = np.linalg.norm(right)
    if not n > 1e-12:
        raise ValueError("look_at: up is parallel to the viewing direction")
    right = right / n
    down = np.cross(forward, right)
    R = np.stack([right, down, forward]) + 0.0          # (no negative zeros)
    return R.astype(np.float32), (-R @ position).astype(np.float32)


def _moved(a, R, t=None):
    """a @ R.T (+ t) spelled out per column — float32 products added left to right, then t — so that numpy and torch,
    on any device, give the same bits (a matrix product is free to order and fuse its sums)."""
    cols = []
    for k in range(3):
        c = (a[..., 0] * float(R[k, 0]) + a[..., 1] * float(R[k, 1])) + a[..., 2] * float(R[k, 2])
        cols.append(c if t is None else c + float(t[k]))
    return cols


def light_arrays(tri, nrm, R, t):
    """Light-frame vertices ``tri @ R.T + t`` and normals ``nrm @ R.T``, float32 [T, 3, 3] each, from numpy arrays
    (numpy results) or torch tensors (results on the tensors' device)."""
    R, t = np.asarray(R, np.float32).reshape(3, 3), np.asarray(t, np.float32).reshape(3)
    if type(tri).__module__.split(".")[0] == "torch":
        import torch
        tri, nrm = tri.to(torch.float32), nrm.to(device=tri.device, dtype=torch.float32)
        return torch.stack(_moved(tri, R, t), -1).contiguous(), torch.stack(_moved(nrm, R), -1).contiguous()
    tri, nrm = np.asarray(tri, np.float32), np.asarray(nrm, np.float32)
    return np.stack(_moved(tri, R, t), -1), np.stack(_moved(nrm, R), -1)
