"""Device time of the environment pass (k_env_shade, csrc/envmap.hip): crender_env_shade between two HIP events, mean
of 50 passes over the same frame, for T-Rex at 1024^2 and at 4096^2 under a random 512^2 cube with its chain, for the six
instances: reflections, the background, and both, each from one level (level 0) and from two (level 0.5).  (The pass
rewrites the colours it blends, so the colour plane changes from pass to pass; the work per pass does not depend on the
colours.)

In the same run, on the same frame, two yardsticks: crender_phong_shade with one point light — the same surface point per
covered pixel — and crender_tex_shade perspective-bilinear under a random 709 x 709 texture — the same four texels per
covered pixel.  Every row of the pass carries its ratios to both as `vs_phong` and `vs_tex`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/env_time.py [--scene trex1024]
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
SIDE = 512
POINT = dict(position=(-0.8, -0.5, -0.2), diffuse=0.9, specular=0.5)


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
    rng = np.random.default_rng(1)
    tex = rng.integers(0, 256, (709, 709, 3), dtype=np.uint8)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex)
    f.bind_environment(rng.integers(0, 256, (6, SIDE, SIDE, 3), dtype=np.uint8), mipmaps=True)
    f.render_arrays(tri, col, nrm, clear=True)
    f.environment_pass()                               # settles the frame; the direct calls below repeat the pass
    assert f._order is None                            # (below 2^18 triangles the inputs stay in the caller's order)
    d_uv, d_tex = f._texture
    level0, level1 = f.get_environment_level(0), f.get_environment_level(1)
    winner = f.get_winner_tensor()
    covered = int((winner >= 0).sum())
    distinct = int(torch.unique(winner).numel()) - 1
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    white = (C.c_float * 3)(255.0, 255.0, 255.0)
    eye = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    tint = (C.c_float * 3)(1.0, 1.0, 1.0)
    T = int(tri.shape[0])

    def row(mode, us, **more):
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "distinct_winners": distinct, "mode": mode,
             "device_us": round(us, 2), **more}
        print(json.dumps(r), flush=True)
        return r["device_us"]

    rows, mask = light_rows([POINT])
    lights5 = (C.c_float * 5)(*rows[0])

    def phong():
        _capi.check(lib.crender_phong_shade(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, f.normals_buffer.data_ptr(), lights5, 1, mask,
            0.1, 5, white, 255.0, f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_phong_shade")
    phong_us = row("phong_1_point", _timed(stream, phong))

    def tex_pass():
        _capi.check(lib.crender_tex_shade(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_uv.data_ptr(), d_tex.data_ptr(), 709, 709,
            None, None, f.color_buffer.data_ptr(), size, size, 0, size, _capi.TEX_PERSPECTIVE | _capi.TEX_BILINEAR, st),
            "crender_tex_shade")
    tex_us = row("tex_perspective_bilinear", _timed(stream, tex_pass))

    kinds = {"reflect": _capi.ENV_REFLECT, "background": _capi.ENV_BACKGROUND, "both": _capi.ENV_REFLECT | _capi.ENV_BACKGROUND}
    for kind, flags in kinds.items():
        for two in (False, True):
            def launch():
                _capi.check(lib.crender_env_shade(
                    f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, f.normals_buffer.data_ptr(),
                    level0.data_ptr(), SIDE, level1.data_ptr() if two else None, SIDE // 2 if two else 0, 0.5 if two else 0.0,
                    eye, 1.0, 0.04, tint, 1.0, f.color_buffer.data_ptr(), size, size, 0, size, flags, st), "crender_env_shade")
            us = _timed(stream, launch)
            row(f"env_{kind}_{'two_levels' if two else 'one_level'}", us, vs_phong=round(us / phong_us, 2),
                vs_tex=round(us / tex_us, 2))


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
            print(f"env_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
