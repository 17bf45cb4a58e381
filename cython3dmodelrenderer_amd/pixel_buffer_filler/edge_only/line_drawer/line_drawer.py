"""Interface of the line drawers the wireframe filler takes (reference: line_drawer/line_drawer.py)."""
from abc import abstractmethod


class LineDrawer:
    @abstractmethod
    def draw_line(self, p1, p2, image, color):
        """Call ``image.set_pixel(x, y, color)`` for every pixel of the line from ``p1`` to ``p2``."""
