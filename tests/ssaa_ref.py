"""Host model of the supersampling resolve: the statements of include/crender_ssaa.h in vectorised numpy, one
float32 operation per step.  The GPU tests compare csrc/resolve.hip with it bit for bit; tests/test_ssaa_cpu.py pins
it by hand."""
import numpy as np

MAX_FACTOR = 8
INT_MIN = np.int32(-2147483648)


def present_u8(image, flip_rows=False):
    """crender_present_u8's cast (run.py:26's astype('uint8') on x86-64): truncate toward zero to int32, INT_MIN
    for a NaN and for anything outside int32, keep the low byte."""
    f = np.asarray(image, np.float32)
    i = np.full(f.shape, INT_MIN, np.int32)
    with np.errstate(invalid="ignore"):
        ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
    i[ok] = np.trunc(f[ok]).astype(np.int32)
    out = (i & 0xFF).astype(np.uint8)
    return np.ascontiguousarray(out[::-1]) if flip_rows else out


def shade(color, normals, light_direction):
    """A shaded copy of `color`: ``GuroIllumination(light_direction).draw_illumination`` by the oracle's statements
    (`light_direction` is what that class is constructed with, as in tests/tex_ref.py)."""
    from oracle import oracle as O
    out = np.array(color, np.float32, copy=True, order="C")
    O.guro(out, np.ascontiguousarray(normals, np.float32), light_direction)
    return out


def resolve(color, s, normals=None, light_direction=None, dtype="float32", flip_rows=False, Y0=0, Y1=None, out=None):
    """crender_ssaa_resolve over output rows Y0 .. Y1: a new [H/s, W/s, 3] array (zeros outside the rows), or
    `out` with those rows replaced."""
    src = np.asarray(color, np.float32)
    H, W = src.shape[:2]
    assert 1 <= s <= MAX_FACTOR and H % s == 0 and W % s == 0 and dtype in ("float32", "uint8")
    if light_direction is not None:
        src = shade(src, normals, light_direction)
    with np.errstate(all="ignore"):
        acc = src[0::s, 0::s]
        for j in range(s):
            for i in range(s):
                if j or i:
                    acc = acc + src[j::s, i::s]
        r = acc / np.float32(s * s)
    assert r.dtype == np.float32
    if dtype == "uint8":
        r = present_u8(r)
    Ho = H // s
    Y1 = Ho if Y1 is None else Y1
    if out is None:
        out = np.zeros(r.shape, r.dtype)
    rows = np.arange(Y0, Y1)
    out[(Ho - 1 - rows) if flip_rows else rows] = r[Y0:Y1]
    return out


def resolve_by_loops(color, s):
    """The same statements pixel by pixel in Python scalars of float32: what the vectorised form is pinned on."""
    src = np.asarray(color, np.float32)
    H, W, C = src.shape
    out = np.empty((H // s, W // s, C), np.float32)
    with np.errstate(all="ignore"):
        for Y in range(H // s):
            for X in range(W // s):
                for c in range(C):
                    acc = src[Y * s, X * s, c]
                    for j in range(s):
                        for i in range(s):
                            if j or i:
                                acc = np.float32(acc + src[Y * s + j, X * s + i, c])
                    out[Y, X, c] = np.float32(acc / np.float32(s * s))
    return out
