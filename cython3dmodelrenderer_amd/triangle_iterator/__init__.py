"""The orders in which the py ``Renderer`` hands a model's triangles to its filler (the reference's
crender/cy/triangle_iterator; the crender/py copy is the same).

Every iterator yields the ``model.get_triangle(i)`` tuples (vertices, colours or None, normals):
``SimpleIterator`` for i = 0 .. T-1, ``DepthIterator`` nearest first — ascending by the smallest vertex
z of each triangle, equal keys kept in index order (a stable sort; -0 and +0 compare equal).

``draw_order(model)`` is the hook of the device path: the permutation the iterator visits the triangles
in, worked out from the ``_vertices_by_triangles`` array alone (a ``Model`` or a ``DeviceModel``, which
has no ``get_triangle``), without building the tuples.  ``None`` means index order.
"""
from __future__ import annotations

from abc import abstractmethod

import numpy as np


def _nearest_first(min_z):
    """Stable ascending permutation of the per-triangle minimum vertex z (float32)."""
    return np.argsort(np.asarray(min_z, np.float32), kind="stable")


class TriangleIterator:
    """Base of the iterators: ``__next__`` returns one triangle's tuple or raises StopIteration."""

    def __iter__(self):
        return self

    @abstractmethod
    def __next__(self):
        pass

    @classmethod
    def draw_order(cls, model):
        raise NotImplementedError(f"{cls.__name__} has no draw order hook: iterate it")


class SimpleIterator(TriangleIterator):
    """The triangles in index order, fetched one at a time."""

    def __init__(self, model):
        self._source = model
        self._total = model.n_triangles()
        self._next = 0

    def __len__(self):
        return self._total

    def __next__(self):
        i = self._next
        if i >= self._total:
            raise StopIteration
        self._next = i + 1
        return self._source.get_triangle(i)

    @classmethod
    def draw_order(cls, model):
        return None


class DepthIterator(TriangleIterator):
    """The triangles nearest first; every tuple is fetched up front to sort them."""

    def __init__(self, model):
        fetched = [model.get_triangle(i) for i in range(model.n_triangles())]
        order = _nearest_first([np.min(vertices[:, 2]) for vertices, _, _ in fetched])
        self._queue = [fetched[i] for i in order]
        self._next = 0

    def __len__(self):
        return len(self._queue)

    def __next__(self):
        if self._next >= len(self._queue):
            raise StopIteration
        self._next += 1
        return self._queue[self._next - 1]

    @classmethod
    def draw_order(cls, model):
        v = model._vertices_by_triangles
        if hasattr(v, "detach"):                       # a DeviceModel's torch tensor
            v = v.detach().cpu().numpy()
        return _nearest_first(np.asarray(v)[:, :, 2].min(axis=1))


__all__ = ["TriangleIterator", "SimpleIterator", "DepthIterator"]
