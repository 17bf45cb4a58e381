"""Device time of the shadow pass (csrc/shadow.hip): crender_shadow_shade between two HIP events, mean of 50 passes over
the same two frames, for T-Rex at 1024^2 under a 1024^2 map and at 4096^2 under a 2048^2 map, the light turned 40 degrees
about y around the model's centre, at K = 1, 3 and 5, with and without the light's winner plane.  (The pass multiplies the
colours it shadows, so the colour plane darkens from pass to pass; the work per pass does not depend on the colours.)

In the same run, on the same camera frame, two yardsticks: crender_tex_shade perspective-nearest under a random 709 x 709
texture — the same gathers per winner, one texel instead of K^2 taps — and crender_guro_illumination.  Every shadow row
carries its ratio to the first as `vs_tex`; the rows of K = 3 and 5 carry the time per tap added to K = 1 as `ns_per_tap`.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/shadow_time.py [--scene trex1024]
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP = 50, 5
SCENES = {"trex1024": (1024, 1024), "trex4096": (4096, 2048)}        # frame side, map side
CHILD_SECONDS = 240


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
    from cython3dmodelrenderer_amd import _capi, scenes, shadow
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size, side = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    with np.load(os.path.join(scenes.GOLDEN_DIR, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    tex = np.random.default_rng(1).integers(0, 256, (709, 709, 3), dtype=np.uint8)
    a = math.radians(40.0)
    R = np.float32([[math.cos(a), 0, -math.sin(a)], [0, 1, 0], [math.sin(a), 0, math.cos(a)]])
    centre = tri.reshape(-1, 3).mean(0, dtype=np.float32)
    ltri, lnrm = shadow.light_arrays(tri, nrm, R, centre - R @ centre)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    g = AdvancedPixelBufferFiller(side, side, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex)
    f.render_arrays(tri, col, nrm, clear=True)
    g.render_arrays(ltri, col, lnrm, clear=True)
    f.bind_shadow_map(g, ltri)
    before = f.get_color_tensor().clone()
    f.shadow_pass()                                    # settles both frames; the direct calls below repeat the pass
    assert f._order is None and g._order is None       # (below 2^18 triangles the inputs stay in the caller's order)
    touched = int((f.get_color_tensor() != before).any(2).sum())
    d_ltri = f._shadow[1]
    d_uv, d_tex = f._texture
    winner = f.get_winner_tensor()
    covered = int((winner >= 0).sum())
    distinct = int(torch.unique(winner).numel()) - 1
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    light = (C.c_float * 3)(-0.28, 0.19, -0.94)
    T = int(tri.shape[0])

    def row(mode, us, **more):
        r = {"scene": name, "map": side, "T": T, "covered": round(covered / npix, 3), "distinct_winners": distinct,
             "shadowed_at_K1": round(touched / max(covered, 1), 3), "mode": mode, "device_us": round(us, 2), **more}
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
    row("illumination_pass_alone", _timed(stream, guro))

    for with_winner in (False, True):
        k1_us = None
        for K in _capi.SHADOW_PCF:
            def launch():
                _capi.check(lib.crender_shadow_shade(
                    f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_ltri.data_ptr(), g._P,
                    g.z_buffer.data_ptr(), g.winner_buffer.data_ptr() if with_winner else None, side, side, 1e-3, 0.25, K,
                    f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_shadow_shade")
            us = _timed(stream, launch)
            more = {"vs_tex": round(us / tex_us, 2)}
            if K == 1:
                k1_us = us
            else:
                more["ns_per_tap"] = round((us - k1_us) * 1000.0 / (K * K - 1), 1)
            row(f"shadow_K{K}" + ("_winner" if with_winner else ""), us, **more)


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
            print(f"shadow_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
