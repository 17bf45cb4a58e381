"""Tap tables of the ambient-occlusion pass (``AdvancedPixelBufferFiller.ao_pass``, include/crender_ao.h)."""
import math

GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def taps(radius_px, n):
    """Exactly `n` distinct integer offsets (dx, dy), none of them (0, 0), all with |dx| and |dy| <= `radius_px`,
    spread over the disc of that radius by a deterministic rule:

    1. the golden-angle spiral: point k of n sits at the radius ``radius_px * sqrt((k + 0.5) / n)`` (equal areas
       between consecutive rings) and the angle ``k * GOLDEN_ANGLE``, and is rounded to the nearest integers; a point
       that rounds to (0, 0) or onto an offset already taken is dropped;
    2. the top-up, while fewer than n are taken: of the offsets of the square not yet taken, the one farthest (in
       Euclidean distance) from its nearest taken offset and from the centre, offsets inside the disc before the
       square's corners; ties go to the smaller (dy, dx).

    Raises ValueError if the square of side 2 * radius_px + 1 holds fewer than n offsets besides its centre."""
    if isinstance(radius_px, bool) or not isinstance(radius_px, int) or radius_px < 1:
        raise ValueError(f"radius_px must be a positive int, got {radius_px!r}")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"the number of taps must be a positive int, got {n!r}")
    room = (2 * radius_px + 1) ** 2 - 1
    if n > room:
        raise ValueError(f"{n} taps do not fit radius_px={radius_px}: the square holds {room} offsets besides (0, 0)")
    out = []
    seen = {(0, 0)}
    for k in range(n):
        r = radius_px * math.sqrt((k + 0.5) / n)
        a = k * GOLDEN_ANGLE
        p = (int(round(r * math.cos(a))), int(round(r * math.sin(a))))
        if p not in seen:
            seen.add(p)
            out.append(p)
    if len(out) < n:
        square = [(dx, dy) for dy in range(-radius_px, radius_px + 1) for dx in range(-radius_px, radius_px + 1)]
        while len(out) < n:
            best, best_key = None, None
            for dx, dy in square:
                if (dx, dy) in seen:
                    continue
                gap = min((dx - sx) ** 2 + (dy - sy) ** 2 for sx, sy in seen)
                key = (dx * dx + dy * dy <= radius_px * radius_px, gap)
                if best_key is None or key > best_key:
                    best, best_key = (dx, dy), key
            seen.add(best)
            out.append(best)
    return out
