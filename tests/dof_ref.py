"""The host model of the depth-of-field pass (include/crender_dof.h, "Depth of field"): the contract's statements in
numpy, one array operation per float32 operation, in the contract's order.  The GPU tests compare the kernel with it bit
for bit; tests/test_dof_cpu.py pins it by identities and against its own float64 evaluation (``dtype=np.float64``: the
same statements from the same float32 inputs, every intermediate in double)."""
import numpy as np

MAX_RADIUS = 12


def view_depth(P, z, dtype=np.float32):
    """zv = P14 / (z - P10), the contract's statement."""
    P16 = np.asarray(P, np.float32).reshape(16)
    with np.errstate(all="ignore"):
        return dtype(P16[14]) / (np.asarray(z, np.float32).astype(dtype) - dtype(P16[10]))


def coc(winner, z, T, P, focus, band, aperture, max_radius, y0=0, y1=None, dtype=np.float32):
    """(s, ia) of every pixel of the frame: the signed circle of confusion and the reciprocal of its footprint; NaN outside
    the rows y0 .. y1."""
    d = dtype
    H, W = winner.shape
    y1 = H if y1 is None else y1
    focus, band, aperture, Rf = d(np.float32(focus)), d(np.float32(band)), d(np.float32(aperture)), d(max_radius)
    pi = d(np.float32(3.14159265358979323846))
    with np.errstate(all="ignore"):
        zv = view_depth(P, z, d)
        dd = zv - focus
        dd = np.where(dd > band, dd - band, np.where(dd < -band, dd + band, d(0)))
        covered = (winner >= 0) & (winner.astype(np.int64) < T)
        s = np.where(covered, aperture * (dd / zv), aperture).astype(d)
        s = np.where(s > Rf, Rf, np.where(s < -Rf, -Rf, s))
        rows = np.arange(H)[:, None]
        s = np.where((rows >= y0) & (rows < y1), s, d(np.nan)).astype(d)
        ia = d(1) / (d(1) + pi * (s * s))
    return s, ia.astype(d)


def _shifted(a, dx, dy, fill):
    """a[y + dy, x + dx] where that is on the frame, `fill` elsewhere."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return out


def dof_blur(color, winner, z, T, P, focus, aperture=4.0, band=0.0, max_radius=8, y0=0, y1=None, out=None, counts=None,
             dtype=np.float32, prune=True, mask=None):
    """The plane crender_dof_blur leaves: `out` (zeros without one) with the rows y0 .. y1 written.  `counts`, a dict,
    receives covered (pixels of the rows with a winner in [0, T)), blurred (pixels of the rows that are not copied), copied,
    taps_taken (the centre included) and largest_c; `mask`, a bool plane, receives which pixels are blurred.  With `prune`
    the offsets beyond ceil(the largest c of the frame) are passed over: none of them is taken (the contract's last consequence), which test_dof_cpu.py checks against the full
    window."""
    d = dtype
    color = np.asarray(color, np.float32)
    winner = np.asarray(winner, np.int32)
    H, W = winner.shape
    y1 = H if y1 is None else y1
    assert 1 <= max_radius <= MAX_RADIUS and color.shape == (H, W, 3)
    s, ia = coc(winner, z, T, P, focus, band, aperture, max_radius, y0, y1, d)
    c = np.abs(s)
    col = color.astype(d)
    nan = d(np.nan)
    finite_c = c[~np.isnan(c)]
    largest = float(finite_c.max()) if finite_c.size else 0.0
    reach = min(max_radius, int(np.ceil(largest))) if prune else max_radius
    Sw = np.zeros((H, W), d)
    S = np.zeros((H, W, 3), d)
    other = np.zeros((H, W), bool)
    taken = 0
    with np.errstate(all="ignore"):
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                dist = np.sqrt(d(np.float32(dx * dx + dy * dy)))
                sq, iaq = _shifted(s, dx, dy, nan), _shifted(ia, dx, dy, nan)
                cq = np.abs(sq)
                mine = (sq > s) & (c < cq)
                r = np.where(mine, c, cq)
                a = np.where(mine, ia, iaq)
                k = (r + d(1)) - dist
                take = k > 0
                if not take.any():
                    continue
                w = np.where(k < d(1), k, d(1)) * a
                Sw = np.where(take, Sw + w, Sw)
                cqol = _shifted(col, dx, dy, d(0))
                S = np.where(take[..., None], S + w[..., None] * cqol, S)
                if dx or dy:
                    other |= take
                taken += int(take[y0:y1].sum())
        blurred = other & (Sw > 0)
        result = np.where(blurred[..., None], S / Sw[..., None], col)
    res = np.zeros((H, W, 3), d) if out is None else np.array(out, d)
    if d is np.float32:
        # the copied pixels keep their bits (np.where above may quiet a signalling NaN on some hosts)
        result = result.astype(np.float32)
        keep = ~blurred
        result.view(np.uint32)[keep] = color.view(np.uint32)[keep]
    res[y0:y1] = result[y0:y1]
    if counts is not None:
        rows = slice(y0, y1)
        covered = (winner >= 0) & (winner.astype(np.int64) < T)
        counts.update(covered=int(covered[rows].sum()), blurred=int(blurred[rows].sum()),
                      copied=int((~blurred[rows]).sum()), taps_taken=taken, largest_c=largest)
    if mask is not None:
        mask[...] = blurred
    return res
