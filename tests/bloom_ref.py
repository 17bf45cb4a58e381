"""Host model of bloom and tone mapping: the statements of include/crender_bloom.h ("Bloom") in vectorised numpy, one
float32 operation per step.  The GPU tests compare csrc/bloom.hip's k_bloom_rows and k_bloom_finish with it bit for
bit, the scratch plane included; tests/test_bloom_cpu.py pins it by identities and against its own float64 evaluation."""
import numpy as np

from ssaa_ref import present_u8

MAX_RADIUS = 32

# The pinned scenes (tests/test_bloom_cpu.py asserts them on this model, tests/test_bloom_gpu.py uses them): T-Rex and the
# soup of seed 71 at 256^2, the threshold the 0.9 quantile of the frame's largest channel; (bright, copied, glow) by radius.
PINNED_THRESHOLD = {"trex": 102.12265014648438, "soup": 219.90069580078125}
PINNED_COUNTS = {("trex", 1): (6554, 56500, 9036), ("trex", 8): (6554, 46352, 19184), ("trex", 32): (6554, 25989, 39547),
                 ("soup", 1): (6554, 50392, 15144), ("soup", 8): (6554, 7263, 58273), ("soup", 32): (6554, 0, 65536)}
F64_MEASURED = 3.113e-5                 # the largest |float32 - float64| the CPU tests measured with this model


def gaussian(radius, sigma=None):
    """cython3dmodelrenderer_amd.bloom.gaussian's statement."""
    sigma = radius / 3.0 if sigma is None else sigma
    k = np.arange(radius + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def inv_white2(white):
    with np.errstate(over="ignore", divide="ignore"):
        return np.float32(np.float64(1.0) / (np.float64(white) * np.float64(white)))


def lit(a):
    """Not +-0, element by element (a NaN is lit)."""
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    return (bits << bits.dtype.type(1)) != 0


def bright_pass(src, threshold):
    """Rule 1: (bright [H, W, 3], the mask of the bright pixels)."""
    dt = src.dtype.type
    with np.errstate(all="ignore"):
        r, g, b = src[..., 0], src[..., 1], src[..., 2]
        m = r.copy()
        m = np.where(g > m, g, m)
        m = np.where(b > m, b, m)
        k = m - dt(np.float32(threshold))
        on = k > 0
        q = k / m
        bright = np.where(on[..., None], src * q[..., None], dt(0))
    return bright, on


def blur(plane, w, axis):
    """Rules 2 and 3: the taps -R .. R along `axis` in that order, from +0, a multiply then an add each; +0 beyond the ends."""
    R = len(w) - 1
    pad = [(0, 0)] * plane.ndim
    pad[axis] = (R, R)
    P = np.pad(plane, pad)
    n = plane.shape[axis]
    acc = np.zeros_like(plane)
    with np.errstate(all="ignore"):
        for d in range(-R, R + 1):
            acc = acc + plane.dtype.type(w[abs(d)]) * np.take(P, range(R + d, R + d + n), axis=axis)
    return acc


def tone(v, exposure=1.0, tonemap=None, white=np.inf, gamma=1, clamp=None, inv_w2=None):
    """Rules 5 and 6 of every channel of `v`; `inv_w2`: the float the entry takes, instead of `white`."""
    dt = v.dtype.type
    o = v
    with np.errstate(all="ignore"):
        if tonemap == "reinhard" or gamma == 2 or np.float32(exposure) != 1:
            a = v * dt(np.float32(exposure))
            a = np.where(a > 0, a, dt(0))
            a = a * dt(np.float32(1.0 / 255.0))
            L = a
            if tonemap == "reinhard":
                L = (a * (dt(1) + a * dt(inv_white2(white) if inv_w2 is None else np.float32(inv_w2)))) / (dt(1) + a)
            if gamma == 2:
                L = np.sqrt(L)
            o = L * dt(255)
        if clamp is not None:
            o = np.where(o > dt(np.float32(clamp)), dt(np.float32(clamp)), o)
    return o


def bloom(src, threshold=255.0, radius=8, weights=None, intensity=1.0, exposure=1.0, tonemap=None, white=np.inf, gamma=1,
          clamp=None, dtype="float32", flip_rows=False, y0=0, y1=None, out=None, counts=None, scratch=None, compute=np.float32,
          inv_w2=None, mask=None):
    """crender_bloom over rows y0 .. y1 of `src` [H, W, 3]: a new array (zeros outside the rows), or `out` with those rows
    replaced.  `counts` (a dict) receives ``bright`` (pixels of the rows above the threshold), ``copied`` (pixels of the
    rows that rule 4 copies) and ``glow`` (the others); `mask` (bool [H, W]) receives the pixels that glow.  `scratch` (an
    array like `src`) receives hb in its rows y0 .. y1.
    `compute` np.float64 evaluates the same statements in double from the same float32 inputs (and returns float64)."""
    src = np.ascontiguousarray(src, np.float32)
    H, W = src.shape[:2]
    y1 = H if y1 is None else y1
    w = (gaussian(radius) if weights is None else np.ascontiguousarray(weights, np.float32)).astype(compute)
    assert 1 <= len(w) - 1 <= MAX_RADIUS and 0 <= y0 < y1 <= H and dtype in ("float32", "uint8")
    if clamp is None and dtype == "uint8":
        clamp = 255.0
    strip = src[y0:y1].astype(compute)
    bright, on = bright_pass(strip, threshold)
    hb = blur(bright, w, axis=1)
    g = blur(hb, w, axis=0)
    with np.errstate(all="ignore"):
        t = compute(np.float32(intensity)) * g
        dark = ~lit(t).any(axis=2)
        v = np.where(dark[..., None], strip, strip + t)
    o = tone(v, exposure, tonemap, white, gamma, clamp, inv_w2)
    assert o.dtype == compute and hb.dtype == compute
    if counts is not None:
        counts.update(bright=int(on.sum()), copied=int(dark.sum()), glow=int((~dark).sum()))
    if mask is not None:
        mask[y0:y1] = ~dark
    if scratch is not None:
        scratch[y0:y1] = hb
    if dtype == "uint8":
        o = present_u8(o.astype(np.float32))
    if out is None:
        out = np.zeros((H, W, 3), o.dtype)
    rows = np.arange(y0, y1)
    out[(H - 1 - rows) if flip_rows else rows] = o
    return out
