"""Device time of the ambient-occlusion pass (csrc/ao.hip): crender_ao_shade between two HIP events, mean of 50 passes over
the same frame, for T-Rex at 1024^2 and at 4096^2, with 16 taps in 8 pixels and 32 taps in 16 pixels (and 64 taps in 32
pixels at 1024^2), plane and face normals, the rotation on and off.  The world radius is 1.5 times the pixel radius at
the model's depth.  (The pass multiplies the colours it occludes, so the colour plane darkens from pass to pass; the work
per pass does not depend on the colours.)

In the same run, on the same frame, three yardsticks: crender_shadow_shade at K = 5 under a map of the frame's size — 25
taps per covered pixel gathered from global memory, no LDS — crender_tex_shade perspective-nearest under a random
709 x 709 texture, and crender_guro_illumination.  Every occlusion row carries `us_per_tap`, its time over its tap count,
to set beside the shadow pass's time per tap added to K = 1 (`us_per_tap` of the shadow_K5 row); the bytes the pass moves
counted from the code — 8 B of z and winner per staged pixel of every tile and its halo that lies on the frame, 24 B of
colour per occluded pixel — and the bandwidth they make of the time.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/ao_time.py [--scene trex1024]
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
SCENES = {"trex1024": 1024, "trex4096": 4096}
SETTINGS = {"trex1024": [(16, 8), (32, 16), (64, 32)], "trex4096": [(16, 8), (32, 16)]}      # taps, radius_px
CHILD_SECONDS = 240
TILE = 32                                      # kTile of csrc/ao.hip


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


def staged_pixels(size, R):
    """Pixels of the frame that the tiles of a size x size frame stage, halos included."""
    spans = [min(size, t * TILE + TILE + R) - max(0, t * TILE - R) for t in range((size + TILE - 1) // TILE)]
    return sum(spans) ** 2


def measure(name):
    import numpy as np
    import torch
    from cython3dmodelrenderer_amd import _capi, ambient_occlusion, scenes, shadow
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    with np.load(os.path.join(scenes.GOLDEN_DIR, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    tex = np.random.default_rng(1).integers(0, 256, (709, 709, 3), dtype=np.uint8)
    a = math.radians(40.0)
    R = np.float32([[math.cos(a), 0, -math.sin(a)], [0, 1, 0], [math.sin(a), 0, math.cos(a)]])
    centre = tri.reshape(-1, 3).mean(0, dtype=np.float32)
    ltri, lnrm = shadow.light_arrays(tri, nrm, R, centre - R @ centre)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    g = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex)
    g.render_arrays(ltri, col, lnrm, clear=True)
    f.bind_shadow_map(g, ltri)
    pixel = float(centre[2]) * 2.0 / (size * 2.4142137)        # a pixel's width at the model's depth
    occluded = {}
    for taps, rpx in SETTINGS[name]:
        for normals in ("plane", "face"):
            for rotate in (True, False):
                f.render_arrays(tri, col, nrm, clear=True)
                before = f.get_color_tensor().clone()
                f.ao_pass(radius=1.5 * rpx * pixel, radius_px=rpx, taps=taps, normals=normals, rotate=rotate)
                occluded[taps, normals, rotate] = int((f.get_color_tensor() != before).any(2).sum())
    f.render_arrays(tri, col, nrm, clear=True)
    f.shadow_pass()                                    # settles both frames; the direct calls below repeat the passes
    assert f._order is None and g._order is None       # (below 2^18 triangles the inputs stay in the caller's order)
    d_ltri = f._shadow[1]
    d_uv, d_tex = f._texture
    winner = f.get_winner_tensor()
    covered = int((winner >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    light = (C.c_float * 3)(-0.28, 0.19, -0.94)
    T = int(tri.shape[0])

    def row(mode, us, **more):
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "mode": mode, "device_us": round(us, 2), **more}
        print(json.dumps(r), flush=True)
        return r["device_us"]

    def tex_pass():
        _capi.check(lib.crender_tex_shade(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_uv.data_ptr(), d_tex.data_ptr(), 709, 709,
            None, None, f.color_buffer.data_ptr(), size, size, 0, size, _capi.TEX_PERSPECTIVE, st), "crender_tex_shade")
    row("tex_perspective_nearest", _timed(stream, tex_pass))

    def guro():
        _capi.check(lib.crender_guro_illumination(f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(), light, size,
                                                  size, 0, size, st), "crender_guro_illumination")
    row("illumination_pass_alone", _timed(stream, guro))

    shadow_us = {}
    for K in (1, 5):
        def launch():
            _capi.check(lib.crender_shadow_shade(
                f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_ltri.data_ptr(), g._P,
                g.z_buffer.data_ptr(), None, size, size, 1e-3, 0.25, K, f.color_buffer.data_ptr(), size, size, 0, size, 0, st),
                "crender_shadow_shade")
        shadow_us[K] = _timed(stream, launch)
        more = {} if K == 1 else {"us_per_tap": round((shadow_us[5] - shadow_us[1]) / 24, 3),
                                  "us_over_all_25_taps": round(shadow_us[5] / 25, 3)}
        row(f"shadow_K{K}", shadow_us[K], **more)

    for taps, rpx in SETTINGS[name]:
        table = ambient_occlusion.taps(rpx, taps)
        taps2 = (C.c_int8 * (2 * taps))(*[v for p in table for v in p])
        for normals in ("plane", "face"):
            for rotate in (True, False):
                flags = (_capi.AO_ROTATE if rotate else 0) | (_capi.AO_FACE_NORMALS if normals == "face" else 0)

                def launch():
                    _capi.check(lib.crender_ao_shade(
                        f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P,
                        f.normals_buffer.data_ptr(), taps2, taps, rpx, 1.5 * rpx * pixel, 0.1, 2.0, 0.0,
                        f.color_buffer.data_ptr(), size, size, 0, size, flags, st), "crender_ao_shade")
                us = _timed(stream, launch)
                occ = occluded[taps, normals, rotate]
                nbytes = staged_pixels(size, rpx) * 8 + occ * 24
                row(f"ao_{taps}_taps_{rpx}_px_{normals}" + ("_rotate" if rotate else ""), us,
                    occluded=round(occ / max(covered, 1), 3), us_per_tap=round(us / taps, 3),
                    vs_shadow_K5=round(us / shadow_us[5], 2), mbytes_counted=round(nbytes / 1e6, 1),
                    gbytes_per_s=round(nbytes / us / 1e3, 1))


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
            print(f"ao_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
