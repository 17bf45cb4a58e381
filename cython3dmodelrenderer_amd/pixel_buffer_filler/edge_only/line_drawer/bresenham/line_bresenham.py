"""Bresenham's line on the host, pixel for pixel the reference's
(line_drawer/bresenham/line_bresenham.py:6-45).

The reference keeps a float error term that starts at ``el / 2`` and moves by whole numbers, so
every value it takes is a multiple of one half: doubled, it is exact integer arithmetic, which is
what this loop runs.  Along the major axis (x if ``|dx| > |dy|``, else y: ties go to y) the line
advances every step; the minor axis advances on the steps where the error drops below zero.
``el + 1`` pixels are set, the start pixel first.  The device form of the same line is
csrc/wireframe.hip."""
from ..line_drawer import LineDrawer


def _sign(v):
    return (v > 0) - (v < 0)


class LineBresenham(LineDrawer):
    def draw_line(self, p1, p2, image, color):
        x, y = p1
        x2, y2 = p2
        sx, sy = _sign(x2 - x), _sign(y2 - y)
        ax, ay = abs(x2 - x), abs(y2 - y)
        if ax > ay:
            el, es, straight = ax, ay, (sx, 0)
        else:
            el, es, straight = ay, ax, (0, sy)
        err2 = el                       # 2 * (el / 2)
        image.set_pixel(x, y, color)
        for _ in range(el):
            err2 -= 2 * es
            if err2 < 0:
                err2 += 2 * el
                x += sx
                y += sy
            else:
                x += straight[0]
                y += straight[1]
            image.set_pixel(x, y, color)
