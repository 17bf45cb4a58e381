"""Cube maps for ``AdvancedPixelBufferFiller.bind_environment``: host numpy only, evaluated in float64, with no parity
claim (what the device does with a cube is stated in include/crender_env.h, "Environment mapping").

A cube is uint8 [6, S, S, 3], the faces in the order +x, -x, +y, -y, +z, -z of the camera's frame under the identity
orientation: x grows with the column, y with the ROW (so +y is down and the sky is around -y), z goes into the screen.
Texel (row i, column j) of a face is centred at ``s = (2 j + 1) / S - 1``, ``t = (2 i + 1) / S - 1``."""
import numpy as np

FACES = ("+x", "-x", "+y", "-y", "+z", "-z")


def face_direction(face, s, t):
    """The direction (dx, dy, dz), its major magnitude 1, that the pass's table sends to `face` (0 .. 5) with
    ``sc / ma = s`` and ``tc / ma = t``: the inverse of that table.  `s` and `t` are numbers or arrays of one shape."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    one = np.ones_like(s)
    if not 0 <= int(face) <= 5:
        raise ValueError(f"face must be 0 .. 5 (+x, -x, +y, -y, +z, -z), got {face!r}")
    return ((one, t, -s), (-one, t, s), (s, one, -t), (s, -one, t), (s, t, one), (-s, t, -one))[int(face)]


def _texel_directions(S):
    """[6, S, S, 3] float64: the direction of every texel's centre."""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= S <= 8192:
        raise ValueError(f"S must be an int from 1 to 8192, got {S!r}")
    c = (2.0 * np.arange(S) + 1.0) / S - 1.0
    t, s = np.meshgrid(c, c, indexing="ij")
    return np.stack([np.stack(face_direction(k, s, t), -1) for k in range(6)])


def cube_from_equirect(image_u8, S):
    """uint8 [6, S, S, 3] from a latitude-longitude panorama uint8 [Hp, Wp, 3]: row 0 is straight up (-y), the last row
    straight down, the middle column is the +z axis and the longitude grows towards +x, wrapping at -z.  Every texel takes
    the bilinear sample of the panorama at its centre's direction (the columns wrap, the rows are clamped), in float64,
    rounded to the nearest byte."""
    img = np.asarray(image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] < 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image_u8 must be uint8 [Hp, Wp, 3], got {img.dtype} {img.shape}")
    d = _texel_directions(S)
    Hp, Wp = img.shape[:2]
    lon = np.arctan2(d[..., 0], d[..., 2])
    lat = np.arcsin(-d[..., 1] / np.sqrt((d * d).sum(-1)))
    fx = (lon / (2.0 * np.pi) + 0.5) * Wp - 0.5
    fy = (0.5 - lat / np.pi) * Hp - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    c0, c1 = x0.astype(np.int64) % Wp, (x0.astype(np.int64) + 1) % Wp
    r0, r1 = np.clip(y0.astype(np.int64), 0, Hp - 1), np.clip(y0.astype(np.int64) + 1, 0, Hp - 1)
    p = img[:, :, :3].astype(np.float64)
    out = (p[r0, c0] * (1 - ax) + p[r0, c1] * ax) * (1 - ay) + (p[r1, c0] * (1 - ax) + p[r1, c1] * ax) * ay
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def gradient_sky(S, zenith=(60, 110, 220), horizon=(200, 220, 240), ground=(70, 60, 50)):
    """uint8 [6, S, S, 3], a procedural sky: with ``u = -dy / |d|`` the height of a texel's direction above the horizon
    (1 straight up), the colour is `horizon` blended towards `zenith` by u above it and towards `ground` by -u below."""
    d = _texel_directions(S)
    u = (-d[..., 1] / np.sqrt((d * d).sum(-1)))[..., None]
    z, h, g = (np.asarray(c, np.float64).reshape(3) for c in (zenith, horizon, ground))
    out = np.where(u >= 0, h + (z - h) * u, h + (g - h) * -u)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)
