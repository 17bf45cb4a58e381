"""``Buffer`` of the reference's crender/py (data_structures/buffer.py): one [height][width][dim] numpy
plane of a given dtype, reset to a fill value by ``clear``.  Indexing goes straight to the array.
``write_to_file`` writes, through PIL, the pixels ``cv2.imwrite(name, buffer[::-1])`` writes: rows
flipped, three channels taken as BGR."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def _on_axis(v, n):
    """v names one of the n pixels 0 .. n-1 of an axis (an integral value; anything else does not)."""
    try:
        return 0 <= v < n and int(v) == v
    except (TypeError, ValueError, OverflowError):
        return False


class Buffer:
    def __init__(self, height: int, width: int, dim: int = 3, dtype: str = 'float32', init_val=0):
        self._height, self._width, self._dim = height, width, dim
        self._dtype, self._init_val = dtype, init_val
        self._buffer = None
        self.clear()

    def clear(self) -> None:
        """A fresh plane holding the fill value (assigned, so numpy's assignment casts it)."""
        plane = np.empty((self._height, self._width, self._dim), dtype=self._dtype)
        plane[...] = self._init_val
        self._buffer = plane

    def __getitem__(self, index) -> np.ndarray:
        return self._buffer[index]

    def __setitem__(self, index, value) -> None:
        self._buffer[index] = value

    def get_size(self) -> Tuple[int, int]:
        return self._height, self._width

    def get_image(self) -> np.ndarray:
        return self._buffer

    def get_pixel(self, x: int, y: int) -> np.ndarray:
        return self._buffer[y, x]

    def set_pixel(self, x: int, y: int, value) -> None:
        """Pixels off the plane are dropped."""
        if _on_axis(x, self._width) and _on_axis(y, self._height):
            self._buffer[y, x] = value

    def write_to_file(self, filename: str) -> None:
        """8-bit planes only (cv2 would convert other depths); 1 channel: grey, 3: BGR, 4: BGRA."""
        from PIL import Image
        rows = self._buffer[::-1]
        if rows.dtype != np.uint8:
            raise TypeError(f"write_to_file writes uint8 buffers, this one is {rows.dtype}")
        channels = {1: ([0], "L"), 3: ([2, 1, 0], "RGB"), 4: ([2, 1, 0, 3], "RGBA")}
        if self._dim not in channels:
            raise ValueError(f"write_to_file writes 1, 3 or 4 channels, not {self._dim}")
        pick, mode = channels[self._dim]
        pixels = np.ascontiguousarray(rows[..., pick])
        Image.fromarray(pixels[..., 0] if mode == "L" else pixels, mode=mode).save(filename)
