#!/usr/bin/env python3
"""Writes tests/golden/trex_uv.npz: the T-Rex's texture coordinates (``uv`` float32 [7347, 2]) and its
faces' texture indices (``faces_uv`` int32 [13814, 3]), parsed from the reference checkout's T-Rex.obj
with this repository's ``Model``.  The texture image itself (870 KB) is not committed; the tests draw
seeded random textures.

Before writing, the script proves that the uv belong to trex_inputs.npz's triangle order: nearest
sampling of the real texture at the vertices' uv must reproduce that fixture's ``col`` bit for bit.

  REFERENCE_ROOT=/path/to/reference python scripts/make_tex_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cython3dmodelrenderer_amd.data_structures.model import Model   # noqa: E402
from cython3dmodelrenderer_amd import scenes                         # noqa: E402
import tex_ref                                                       # noqa: E402

REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")


def main():
    trex = Model.read_model(os.path.join(REF, "objects", "T-Rex.obj"))
    uv_t = trex.get_texture_coords_by_triangles()
    tex = trex.get_texture()
    assert uv_t is not None and tex is not None, "the T-Rex did not load with its texture"
    _, col, _ = scenes.load_fixture("trex_inputs.npz")
    flat = uv_t.reshape(-1, 2)
    sampled = tex_ref.nearest(flat[:, 0], flat[:, 1], tex).reshape(col.shape)
    assert np.array_equal(sampled.view(np.uint32), col.view(np.uint32)), \
        "nearest sampling at the vertices does not reproduce trex_inputs.npz's colours"
    uv = np.ascontiguousarray(trex._texture_coords[:, :2], dtype=np.float32)
    faces_uv = np.asarray(trex._triangles_texture_coords, dtype=np.int32)
    assert np.array_equal(uv[faces_uv], uv_t)
    path = os.path.join(OUT, "trex_uv.npz")
    np.savez_compressed(path, uv=uv, faces_uv=faces_uv)
    print(f"{path}: uv {uv.shape}, faces_uv {faces_uv.shape}, texture {tex.shape}, {os.path.getsize(path)} bytes; "
          "vertex colours of trex_inputs.npz reproduced bit for bit")


if __name__ == "__main__":
    main()
