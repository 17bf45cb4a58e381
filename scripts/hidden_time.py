"""Device time of the hidden-line pass (csrc/wireframe.hip, k_wire_hidden<mark> and <resolve>): crender_wire_hidden between
two HIP events, mean of 50 calls over the same frame, for T-Rex at 1024^2 and at 4096^2, with all edges and with the
30-degree feature mask, dashed (4, 4) under the winner rule at bias 1e-3.  The marks depend on z, the winner plane and the
triangles alone, never on the colours the pass writes, so every repetition does the same work.

Next to it, in the same run, on the same frame, two yardsticks of the same translation unit: crender_wire_overlay (all
edges, width 1, no fill: one projected triangle per covered pixel) and crender_wire_draw (the wireframe filler's walker
over the same triangles projected to the screen, one constant colour: the same Bresenham without the depth test and the
key plane).  Every row of the new pass carries its ratios to them as `vs_overlay` and `vs_draw`.  Every row is the mean of
three such measurements and carries their spread (largest minus smallest) as `spread_us`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/hidden_time.py [--scene trex1024]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP, ROUNDS = 50, 5, 3
SCENES = {"trex1024": 1024, "trex4096": 4096}
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


def _on_screen(tri, P, w, h):
    """The triangles projected to pixels, for the wireframe filler, which projects nothing (a yardstick's operand: the
    statements of crender_project in numpy float32, not held to its bits)."""
    v = np.asarray(tri, np.float32).copy()
    P = np.asarray(P, np.float32)
    z = v[..., 2].copy()
    for j in range(3):
        v[..., j] = v[..., 0] * P[0, j] + v[..., 1] * P[1, j] + v[..., 2] * P[2, j] + P[3, j]
    for j in range(3):
        v[..., j] = v[..., j] / z
    v[..., 0] = (v[..., 0] + 1) * np.float32(w / 2.0)
    v[..., 1] = (v[..., 1] + 1) * np.float32(h / 2.0)
    return np.ascontiguousarray(v)


def measure(name):
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    dev = [torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)]
    f.render_arrays(*dev, clear=True)
    mask = torch.from_numpy(feature_edges(tri, 30.0)).to(f.device)
    f.hidden_line_pass()                               # settles the frame and allocates the key plane; the calls below repeat it
    assert f._order is None                            # (below 2^18 triangles the inputs stay in the caller's order)
    covered = int((f.get_winner_tensor() >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    white = (C.c_float * 3)(255.0, 255.0, 255.0)
    black = (C.c_float * 3)(0.0, 0.0, 0.0)
    T = int(tri.shape[0])

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "mode": mode, "device_us": round(us, 2),
             "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    def overlay():
        _capi.check(lib.crender_wire_overlay(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, None, white, None, 1.0, 1.0, 1.0,
            f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_wire_overlay")
    overlay_us = row("wire_overlay_all_w1", _timed(stream, overlay))

    screen = torch.from_numpy(_on_screen(tri, f.proj_mat, size, size)).to(f.device)
    status = torch.zeros(1, dtype=torch.int32, device=f.device)

    def draw():
        _capi.check(lib.crender_wire_draw(
            screen.data_ptr(), None, T, white, None, f.color_buffer.data_ptr(), None, None, size, size, 0, status.data_ptr(),
            st), "crender_wire_draw")
    draw_us = row("wire_draw_const", _timed(stream, draw))
    assert int(status.item()) == 0

    key = f._hidden_key
    for edges_name, edges in (("all", None), ("mask30", mask)):
        def launch():
            _capi.check(lib.crender_wire_hidden(
                f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P,
                None if edges is None else edges.data_ptr(), black, 0.5, 4, 4, 1e-3, key.data_ptr(), f.color_buffer.data_ptr(),
                size, size, 0, size, _capi.WIRE_HIDDEN_USE_WINNER, st), "crender_wire_hidden")
        us, spread = _timed(stream, launch)
        row(f"hidden_{edges_name}", (us, spread), vs_overlay=round(us / overlay_us, 2), vs_draw=round(us / draw_us, 2))
    assert not bool(key.any())                         # every call left the key plane zero


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(SCENES))
    args = ap.parse_args()
    if args.scene:
        measure(args.scene)
        return 0
    for name in SCENES:
        rc = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__),
                             "--scene", name]).returncode
        if rc != 0:
            print(f"hidden_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
