"""``Buffer`` of the reference's crender/py, and its ``Model`` (the cy ``Model``: the reference's py
``Model`` uses ``np.int``, which numpy no longer has, and its ``run.py`` takes the cy one anyway)."""
from ...data_structures import Model
from .buffer import Buffer

__all__ = ["Buffer", "Model"]
