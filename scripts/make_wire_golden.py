"""Fixtures of the wireframe filler from the reference's own code: tests/golden/wire_lines.npz and
tests/golden/wire_golden.json.

Runs the reference checkout's crender/py line drawer, wireframe filler and Buffer, loaded by file
path (cv2 and the package __init__ files are stubbed: nothing else of the reference is imported),
and writes data only:

  wire_lines.npz     3 000 lines of LineBresenham.draw_line — every octant, |dx| == |dy|, zero length,
                     axis-aligned, endpoints up to 5 000 pixels off a 256 x 256 screen: endpoints, the
                     number of set_pixel calls and the sha256 of the int32 (x, y) sequence they made
                     (a logging image), and the whole sequence of the 300 shortest lines
  wire_golden.json   sha256 of the float32 colour plane [h][w][3] that
                     EdgeOnlyPixelBufferFiller.compute_triangle_statistics leaves after every triangle of
                     a fixture in index order (the py Renderer with SimpleIterator), the fixture fitted as
                     Renderer.render(normalize_model=True) fits it (scenes.fit_soup_to_frame), in the
                     modes {edges, dots} x {line_color, forced triangle colours}

usage: python scripts/make_wire_golden.py REFERENCE_ROOT   (a checkout of the reference; or set $REFERENCE_ROOT)
"""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cython3dmodelrenderer_amd import scenes  # noqa: E402

LINE_COLOR = [255.0, 64.5, 3.0]
SCENES = {                 # name -> (fixture, h, w, has colours)
    "cube256": ("cube_inputs.npz", 256, 256, True),
    "trex1024": ("trex_inputs.npz", 1024, 1024, True),
    "bunny1024": ("bunny_inputs.npz", 1024, 1024, False),
}
SCREEN = 256               # the frame wire_lines' endpoints are spread around


def load_reference(ref_root):
    """(LineBresenham, EdgeOnlyPixelBufferFiller, Buffer) of the reference's crender/py."""
    py = os.path.join(ref_root, "crender", "py")
    sys.modules["cv2"] = types.ModuleType("cv2")
    for pkg in ("crender", "crender.py", "crender.py.data_structures", "crender.py.pixel_buffer_filler",
                "crender.py.pixel_buffer_filler.edge_only", "crender.py.pixel_buffer_filler.edge_only.line_drawer"):
        mod = types.ModuleType(pkg)
        mod.__path__ = []
        sys.modules[pkg] = mod

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(py, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    buf = load("crender.py.data_structures.buffer", "data_structures/buffer.py")
    sys.modules["crender.py.data_structures"].Buffer = buf.Buffer
    pbf = load("crender.py.pixel_buffer_filler.pixel_buffer_filler", "pixel_buffer_filler/pixel_buffer_filler.py")
    sys.modules["crender.py.pixel_buffer_filler"].PixelBufferFiller = pbf.PixelBufferFiller
    ld = load("crender.py.pixel_buffer_filler.edge_only.line_drawer.line_drawer",
              "pixel_buffer_filler/edge_only/line_drawer/line_drawer.py")
    sys.modules["crender.py.pixel_buffer_filler.edge_only.line_drawer"].LineDrawer = ld.LineDrawer
    lb = load("crender.py.pixel_buffer_filler.edge_only.line_drawer.bresenham.line_bresenham",
              "pixel_buffer_filler/edge_only/line_drawer/bresenham/line_bresenham.py")
    eo = load("crender.py.pixel_buffer_filler.edge_only.edge_only_pixel_buffer_filler",
              "pixel_buffer_filler/edge_only/edge_only_pixel_buffer_filler.py")
    return lb.LineBresenham, eo.EdgeOnlyPixelBufferFiller, buf.Buffer


class _Log:
    def __init__(self):
        self.px = []

    def set_pixel(self, x, y, value):
        self.px.append((x, y))


def make_lines(LineBresenham, rng):
    S, M = SCREEN, 5000
    p1, p2 = [], []

    def add(a, b):
        p1.append(a)
        p2.append(b)

    def pt(lo, hi):
        return [int(v) for v in rng.integers(lo, hi, 2)]

    for _ in range(1200):                                  # anywhere, all octants
        add(pt(-M, S + M), pt(-M, S + M))
    for _ in range(900):                                   # short lines around the screen
        a = pt(-20, S + 20)
        add(a, [a[0] + int(rng.integers(-40, 41)), a[1] + int(rng.integers(-40, 41))])
    for _ in range(300):                                   # |dx| == |dy|
        a, d = pt(-M, S + M), int(rng.integers(0, 800))
        add(a, [a[0] + d * int(rng.choice([-1, 1])), a[1] + d * int(rng.choice([-1, 1]))])
    for _ in range(100):                                   # zero length
        a = pt(-M, S + M)
        add(a, list(a))
    for _ in range(300):                                   # axis-aligned
        a, d = pt(-M, S + M), int(rng.integers(-900, 901))
        add(a, [a[0] + d, a[1]] if rng.integers(2) else [a[0], a[1] + d])
    for _ in range(200):                                   # |dx| == |dy| +- 1 (next to the tie)
        a, d = pt(-50, S + 50), int(rng.integers(1, 300))
        e = d + int(rng.choice([-1, 1]))
        sx, sy = int(rng.choice([-1, 1])), int(rng.choice([-1, 1]))
        add(a, [a[0] + sx * d, a[1] + sy * e] if rng.integers(2) else [a[0] + sx * e, a[1] + sy * d])
    drawer = LineBresenham()
    lengths, shas, seqs = [], [], []
    for a, b in zip(p1, p2):
        log = _Log()
        drawer.draw_line(list(a), list(b), log, None)
        seq = np.asarray(log.px, dtype=np.int32)
        lengths.append(len(seq))
        shas.append(np.frombuffer(hashlib.sha256(seq.tobytes()).digest(), np.uint8))
        seqs.append(seq)
    lengths = np.asarray(lengths, np.int64)
    full = np.sort(np.argsort(lengths, kind="stable")[:300])
    offsets = np.concatenate([[0], np.cumsum(lengths[full])]).astype(np.int64)
    return dict(p1=np.asarray(p1, np.int32), p2=np.asarray(p2, np.int32), length=lengths, sha=np.stack(shas),
                full_index=full.astype(np.int32), full_offsets=offsets,
                full_xy=np.concatenate([seqs[i] for i in full]).astype(np.int32))


def draw_scene(Filler, LineBresenham, Buffer, tri, col, h, w, edges, forced):
    filler = Filler(LineBresenham(), LINE_COLOR,
                    draw_edges=edges, force_triangle_colors=forced)
    cb = Buffer(h, w, dim=3, dtype="float32")
    zb = Buffer(h, w, dim=1, init_val=1e6, dtype="float32")
    nb = Buffer(h, w, dim=3, dtype="float32")
    for i in range(tri.shape[0]):
        filler.compute_triangle_statistics(tri[i], None if col is None else col[i], None, cb, zb, nb)
    return hashlib.sha256(np.ascontiguousarray(cb.get_image(), np.float32).tobytes()).hexdigest()


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        sys.exit(__doc__)
    LineBresenham, Filler, Buffer = load_reference(ref_root)
    out = os.path.join(ROOT, "tests", "golden")
    lines = make_lines(LineBresenham, np.random.default_rng(20261016))
    np.savez_compressed(os.path.join(out, "wire_lines.npz"), **lines)
    doc = {"line_color": LINE_COLOR, "fit": "scenes.fit_soup_to_frame", "scenes": {}}
    for name, (fixture, h, w, has_col) in SCENES.items():
        tri, col, _ = scenes.load_fixture(fixture)
        fitted = scenes.fit_soup_to_frame(tri, h, w)
        entry = {"fixture": fixture, "h": h, "w": w, "T": int(tri.shape[0]),
                 "vertices_sha": hashlib.sha256(fitted.tobytes()).hexdigest(), "planes": {}}
        for edges in (True, False):
            for forced in ((False, True) if has_col else (False,)):
                key = ("edges" if edges else "dots") + ("_forced" if forced else "_line")
                entry["planes"][key] = draw_scene(Filler, LineBresenham, Buffer, fitted, col if forced else None,
                                                  h, w, edges, forced)
                print(name, key, entry["planes"][key][:16], flush=True)
        doc["scenes"][name] = entry
    with open(os.path.join(out, "wire_golden.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
