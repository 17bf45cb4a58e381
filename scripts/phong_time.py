"""Device time of the Phong pass (csrc/phong.hip): crender_phong_shade between two HIP events, mean of 50 passes over the
same frame, for T-Rex at 1024^2 and at 4096^2, under one point light, one directional light and four lights (two points,
two directions), at shininess 32.  (The pass rewrites the colours it lights, so the colour plane changes from pass to
pass — with the clamp at 255 it saturates; the work per pass does not depend on the colours.)

In the same run, on the same frame, two yardsticks: crender_tex_shade perspective-nearest under a random 709 x 709
texture — the same gathers and the same barycentrics per winner — and crender_guro_illumination, the light this pass
replaces.  Every Phong row carries its ratios to both as `vs_tex` and `vs_guro`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/phong_time.py [--scene trex1024]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 50, 5
SCENES = {"trex1024": 1024, "trex4096": 4096}
CHILD_SECONDS = 240
POINT = dict(position=(-0.8, -0.5, -0.2), diffuse=0.9, specular=0.5)
DIRECTION = dict(direction=(0.3, -0.2, 1.0), diffuse=0.9, specular=0.5)
MODES = {
    "phong_1_point": [POINT],
    "phong_1_direction": [DIRECTION],
    "phong_4_lights": [dict(POINT, diffuse=0.4), dict(DIRECTION, diffuse=0.3), dict(position=(1.5, -2.0, -0.5), diffuse=0.2, specular=0.25),
                       dict(direction=(-1.0, 0.5, 0.25), diffuse=0.1, specular=0.125)],
}


def _timed(stream, launch):
    import torch
    for _ in range(WARMUP):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        launch()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / REPS


def measure(name):
    import numpy as np
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.illumination.phong_illumination import light_rows
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    with np.load(os.path.join(scenes.GOLDEN_DIR, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    tex = np.random.default_rng(1).integers(0, 256, (709, 709, 3), dtype=np.uint8)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex)
    f.render_arrays(tri, col, nrm, clear=True)
    f.phong_pass([POINT])                              # settles the frame; the direct calls below repeat the pass
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
    T = int(tri.shape[0])

    def row(mode, us, **more):
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "distinct_winners": distinct, "mode": mode,
             "device_us": round(us, 2), **more}
        print(json.dumps(r), flush=True)
        return r["device_us"]

    def tex_pass():
        _capi.check(lib.crender_tex_shade(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_uv.data_ptr(), d_tex.data_ptr(), 709, 709,
            None, None, f.color_buffer.data_ptr(), size, size, 0, size, _capi.TEX_PERSPECTIVE, st), "crender_tex_shade")
    tex_us = row("tex_perspective_nearest", _timed(stream, tex_pass))

    def guro():
        _capi.check(lib.crender_guro_illumination(f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(), light, size,
                                                  size, 0, size, st), "crender_guro_illumination")
    guro_us = row("illumination_pass_alone", _timed(stream, guro))

    for mode, lights in MODES.items():
        rows, mask = light_rows(lights)
        lights5 = (C.c_float * (5 * len(rows)))(*[v for r in rows for v in r])

        def launch():
            _capi.check(lib.crender_phong_shade(
                f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, f.normals_buffer.data_ptr(), lights5,
                len(rows), mask, 0.1, 5, white, 255.0, f.color_buffer.data_ptr(), size, size, 0, size, 0, st),
                "crender_phong_shade")
        us = _timed(stream, launch)
        row(mode, us, vs_tex=round(us / tex_us, 2), vs_guro=round(us / guro_us, 2))


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
            print(f"phong_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
