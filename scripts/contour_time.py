"""Device time of the contour classification (csrc/wireframe.hip, k_wire_facing and k_wire_contour_mask):
crender_wire_contours between two HIP events, mean of 50 calls for the view of the same frame, for T-Rex (13 814
triangles, 1024^2) and for a closed sphere of about a million triangles made here (1024^2; at that size the filler keeps
a tile-coherent copy of the triangles, so the call goes through d_pos_of).  The partner table is made once, on the
device (wireframe.edge_partners), outside the timed region; its time is printed beside it (one call, wall clock with a
synchronisation: torch's sort and unique, not this library's code).

In the same run, on the same frame, the yardstick: crender_wire_overlay drawing the mask the call made (over the
colour, width 1).  Every row is the mean of three such measurements and carries their spread (largest minus smallest)
as `spread_us`; the contour rows carry their ratio to the overlay as `vs_overlay`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/contour_time.py [--scene trex]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP, ROUNDS = 50, 5, 3
SCENES = ("trex", "sphere1m")
SIZE = 1024
CHILD_SECONDS = 240


def _timed(stream, launch):
    """(mean, spread) in microseconds of ROUNDS measurements of REPS launches each."""
    import torch
    for _ in range(WARMUP):
        launch()
    got = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(REPS):
            launch()
        b.record(stream)
        b.synchronize()
        got.append(a.elapsed_time(b) * 1000.0 / REPS)
    return sum(got) / len(got), max(got) - min(got)


def sphere(stacks=708, slices=708, radius=0.35, centre=(0.0, 0.0, 1.0)):
    """A closed, consistently wound sphere of 2 * slices * (stacks - 1) triangles (1 001 112 by default) in front of
    the camera: (tri, col, nrm) float32 [T, 3, 3], the normals pointing outwards."""
    import numpy as np
    th = np.linspace(0.0, np.pi, stacks + 1)[1:-1]
    ph = np.arange(slices) * (2.0 * np.pi / slices)
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.cos(th)[:, None] * np.ones_like(ph),
                     np.sin(th)[:, None] * np.sin(ph)], 2).astype(np.float32)          # [stacks - 1, slices, 3]
    nxt = np.roll(ring, -1, 1)
    top = np.broadcast_to(np.float32([0, 1, 0]), (slices, 3))
    bottom = np.broadcast_to(np.float32([0, -1, 0]), (slices, 3))
    a, b, c, d = ring[:-1], nxt[:-1], ring[1:], nxt[1:]
    unit = np.concatenate([np.stack([top, nxt[0], ring[0]], 1), np.stack([bottom, ring[-1], nxt[-1]], 1),
                           np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([b, d, c], 2).reshape(-1, 3, 3)])
    tri = np.ascontiguousarray(unit * np.float32(radius) + np.float32(centre))
    col = np.full_like(tri, 200.0)
    return tri, col, np.ascontiguousarray(unit)


def measure(name):
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.wireframe import edge_partners
    lib = _capi.load()
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz") if name == "trex" else sphere()
    f = AdvancedPixelBufferFiller(SIZE, SIZE, fov=45.0, track_winner=True)
    f.render_arrays(tri, col, nrm, clear=True)
    T = int(tri.shape[0])
    d_tri = torch.from_numpy(tri).to(f.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    partners = edge_partners(d_tri)
    torch.cuda.synchronize()
    table_ms = (time.perf_counter() - t0) * 1e3
    edges = f.contour_edges(partners)                  # (the direct calls below repeat it)
    f.wire_pass(edges=edges)                           # settles the frame
    drawn = int(((edges[:, None] >> torch.arange(3, device=f.device)) & 1).sum())
    pos_of = None if f._order is None else f._order[1].data_ptr()
    facing = torch.empty(T, dtype=torch.int8, device=f.device)
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    white = (C.c_float * 3)(255.0, 255.0, 255.0)

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "size": SIZE, "presorted": pos_of is not None, "contour_half_edges": drawn,
             "partner_table_ms": round(table_ms, 1), "mode": mode, "device_us": round(us, 2), "spread_us": round(spread, 2),
             **more}
        print(json.dumps(r), flush=True)
        return us

    def overlay():
        _capi.check(lib.crender_wire_overlay(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, pos_of, f._P, edges.data_ptr(), white, None, 1.0, 1.0, 1.0,
            f.color_buffer.data_ptr(), SIZE, SIZE, 0, SIZE, 0, st), "crender_wire_overlay")
    overlay_us = row("wire_overlay_of_the_mask_w1", _timed(stream, overlay))

    for mode, flags in (("contours", 0), ("contours_borders", _capi.WIRE_CONTOUR_BORDERS)):
        def launch():
            _capi.check(lib.crender_wire_contours(
                f._inputs[0].data_ptr(), T, pos_of, f._P, partners.data_ptr(), None, facing.data_ptr(), edges.data_ptr(),
                SIZE, SIZE, flags, st), "crender_wire_contours")
        us, spread = _timed(stream, launch)
        row(mode, (us, spread), vs_overlay=round(us / overlay_us, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=SCENES)
    args = ap.parse_args()
    if args.scene:
        measure(args.scene)
        return 0
    for name in SCENES:
        rc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__),
                             "--scene", name]).returncode
        if rc != 0:
            print(f"contour_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
