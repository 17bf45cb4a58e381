"""Device time of the hidden-line overlay (csrc/wireframe.hip, k_wire_overlay): crender_wire_overlay between two HIP
events, mean of 50 passes over the same frame, for T-Rex at 256^2 (where nearly every tap of the outline is a new
triangle), at 1024^2 and at 4096^2: all edges and the 30-degree feature mask, with and without a fill, at width 1 and
width 3 (feather 1).  Next to it, in the same run, the outline (k_wire_outline, crender_wire_outline) at radius 2
(width 1), 4 and 8 (width 3) under the same masks and fills: every outline row carries its ratio to the overlay row of
the same mask, fill and width as `vs_overlay`.  (Without a fill the pass blends the lines over what
it finds, so the colour under a line converges to the line's colour from pass to pass; the work per pass does not depend
on the colours.)

In the same run, on the same frame, two yardsticks: crender_tex_shade perspective-nearest under a random 709 x 709
texture — the same gathers and the same projection per winner, 17 divisions, a store for every covered pixel — and
crender_guro_illumination.  Every row is the mean of three such measurements and carries their spread (largest minus
smallest) as `spread_us`; every overlay row carries its ratios to both yardsticks as `vs_tex` and `vs_guro`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/wire_pass_time.py [--scene trex1024]
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
SCENES = {"trex256": 256, "trex1024": 1024, "trex4096": 4096}
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
    import numpy as np
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.wireframe import feature_edges
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    with np.load(os.path.join(scenes.GOLDEN_DIR, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    tex = np.random.default_rng(1).integers(0, 256, (709, 709, 3), dtype=np.uint8)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex)
    f.render_arrays(tri, col, nrm, clear=True)
    f.wire_pass()                                      # settles the frame; the direct calls below repeat the pass
    assert f._order is None                            # (below 2^18 triangles the inputs stay in the caller's order)
    d_uv, d_tex = f._texture
    winner = f.get_winner_tensor()
    covered = int((winner >= 0).sum())
    distinct = int(torch.unique(winner).numel()) - 1
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    light = (C.c_float * 3)(-0.28, 0.19, -0.94)
    white = (C.c_float * 3)(255.0, 255.0, 255.0)
    grey = (C.c_float * 3)(40.0, 40.0, 40.0)
    T = int(tri.shape[0])
    feature = torch.from_numpy(feature_edges(tri, 30.0)).to(f.device)

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "distinct_winners": distinct, "mode": mode,
             "device_us": round(us, 2), "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    def tex_pass():
        _capi.check(lib.crender_tex_shade(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_uv.data_ptr(), d_tex.data_ptr(), 709, 709,
            None, None, f.color_buffer.data_ptr(), size, size, 0, size, _capi.TEX_PERSPECTIVE, st), "crender_tex_shade")
    tex_us = row("tex_perspective_nearest", _timed(stream, tex_pass))

    def guro():
        _capi.check(lib.crender_guro_illumination(f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(), light, size,
                                                  size, 0, size, st), "crender_guro_illumination")
    guro_us = row("illumination_pass_alone", _timed(stream, guro))

    overlay_us = {}
    for edges_name, edges in (("all", None), ("feature30", feature)):
        for fill_name, fill in (("over", None), ("fill", grey)):
            for width in (1.0, 3.0):
                def launch():
                    _capi.check(lib.crender_wire_overlay(
                        f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P,
                        None if edges is None else edges.data_ptr(), white, fill, width, 1.0, 1.0, f.color_buffer.data_ptr(),
                        size, size, 0, size, 0, st), "crender_wire_overlay")
                us, spread = _timed(stream, launch)
                overlay_us[edges_name, fill_name, width] = us
                row(f"wire_{edges_name}_{fill_name}_w{int(width)}", (us, spread), vs_tex=round(us / tex_us, 2),
                    vs_guro=round(us / guro_us, 2))

    for edges_name, edges in (("all", None), ("feature30", feature)):
        for fill_name, fill in (("over", None), ("fill", grey)):
            for radius, width in ((2, 1.0), (4, 3.0), (8, 3.0)):
                def launch():
                    _capi.check(lib.crender_wire_outline(
                        f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P,
                        None if edges is None else edges.data_ptr(), white, fill, width, 1.0, 1.0, 1e-3, radius,
                        f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_wire_outline")
                us, spread = _timed(stream, launch)
                row(f"outline_{edges_name}_{fill_name}_r{radius}_w{int(width)}", (us, spread),
                    vs_overlay=round(us / overlay_us[edges_name, fill_name, width], 2), vs_tex=round(us / tex_us, 2),
                    vs_guro=round(us / guro_us, 2))


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
            print(f"wire_pass_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
