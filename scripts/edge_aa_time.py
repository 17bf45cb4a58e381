"""Device time of the geometric edge anti-aliasing (csrc/wireframe.hip, k_wire_edge_aa): crender_wire_edge_aa between
two HIP events, mean of 50 passes over the same frame, for T-Rex at 1024^2 and at 4096^2, with all edges and with the mask
of the view (``contour_edges`` over the 30-degree feature mask, borders on).  The pass only reads the frame, so every
repetition does the same work.

Next to it, in the same run, on the same frame: crender_wire_overlay (all edges, width 1, no fill), the pass of the same
unit that gathers and projects one triangle per covered pixel; every row of the new pass carries its ratio to it as
`vs_overlay`.  And what the pass replaces: the frame drawn at twice the size and resolved (``render_arrays`` at 2x, then
``resolve(2)``) against the frame at 1x followed by this pass (``render_arrays``, then ``edge_aa``), both through the
filler's own methods, each with the one synchronisation it makes, between the same two events: `frame_us`, and
`vs_ssaa2` on the rows of the new pass.  Every row is the mean of three such measurements and carries their spread
(largest minus smallest) as `spread_us`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/edge_aa_time.py [--scene trex1024]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

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


def measure(name):
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    dev = [torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)]
    f.render_arrays(*dev, clear=True)
    view = f.contour_edges(edge_partners(tri), static=feature_edges(tri, 30.0), borders=True)
    out = f.edge_aa()                                  # settles the frame; the direct calls below repeat the pass
    assert f._order is None                            # (below 2^18 triangles the inputs stay in the caller's order)
    winner = f.get_winner_tensor()
    covered = int((winner >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    white = (C.c_float * 3)(255.0, 255.0, 255.0)
    T = int(tri.shape[0])

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "mode": mode, "device_us": round(us, 2),
             "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    # ---- the frame at 2x and its resolve, against the frame at 1x and the pass: through the filler's methods
    big = AdvancedPixelBufferFiller(2 * size, 2 * size, fov=45.0, track_winner=True)

    def ssaa2():
        big.render_arrays(*dev, clear=True)
        big.resolve(2)
    ssaa_us = row("frame_2x_then_resolve2", _timed(stream, ssaa2))
    del big

    def plain():
        f.render_arrays(*dev, clear=True)
        f.get_color_tensor()
    row("frame_1x_alone", _timed(stream, plain))
    for edges_name, edges in (("all", None), ("view", view)):
        def frame():
            f.render_arrays(*dev, clear=True)
            f.edge_aa(edges=edges)
        us, spread = _timed(stream, frame)
        row(f"frame_1x_then_edge_aa_{edges_name}", (us, spread), vs_ssaa2=round(us / ssaa_us, 3))

    # ---- the pass alone, through the C entry, against the overlay on the same frame
    f.render_arrays(*dev, clear=True)
    f.edge_aa()

    def overlay():
        _capi.check(lib.crender_wire_overlay(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, None, white, None, 1.0, 1.0, 1.0,
            f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_wire_overlay")
    overlay_us = row("wire_overlay_all_w1", _timed(stream, overlay))
    for edges_name, edges in (("all", None), ("view", view)):
        def launch():
            _capi.check(lib.crender_wire_edge_aa(
                f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P,
                None if edges is None else edges.data_ptr(), out.data_ptr(), f.color_buffer.data_ptr(), size, size, 0, size, 0,
                st), "crender_wire_edge_aa")
        us, spread = _timed(stream, launch)
        row(f"edge_aa_{edges_name}", (us, spread), vs_overlay=round(us / overlay_us, 2))


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
            print(f"edge_aa_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
