"""Device time of the normal-map pass (csrc/normal_map.hip, k_nmap_shade): crender_nmap_shade between two HIP events,
mean of 50 passes over the same frame, for T-Rex at 1024^2 and 4096^2 under the normal map of a random 709 x 709 height
map, each filter x uv mode.  Next to every row, measured in the same run on the same frame: the texture pass with the
same filter (crender_tex_shade, or crender_mip_shade for trilinear) under a random texture of the same size, without a
light — the same gathers and texel fetches; this pass adds the frame arithmetic and reads and writes normals where
that one writes colour — and the illumination pass alone (crender_guro_illumination).  Also crender_nmap_from_height of
the height map.  (The passes of a run perturb the plane the pass before left: every covered pixel is written each time.)

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its
own under ``timeout`` and stops at the first one that fails:

  python scripts/nmap_time.py [--scene trex1024]
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
SCENES = {"trex1024": (1024, 709), "trex4096": (4096, 709)}
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
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size, side = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    with np.load(os.path.join(scenes.GOLDEN_DIR, "trex_uv.npz")) as z:
        uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    rng = np.random.default_rng(1)
    tex = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    height = rng.integers(0, 256, (side, side), dtype=np.uint8)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex, mipmaps=True)
    f.bind_normal_map(height=height, mipmaps=True)
    f.render_arrays(tri, col, nrm, clear=True)
    f.normal_map_pass()                                # settles the frame; the direct calls below repeat the pass
    d_uv, d_tex = f._texture
    d_tex_chain = f._mip[0]
    d_map, d_map_chain = f.get_normal_map(), f._normal_map[2][0]
    assert f._order is None                            # (below 2^18 triangles the inputs stay in the caller's order)
    covered = int((f.get_winner_tensor() >= 0).sum().item())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    T = int(tri.shape[0])
    win, d_tri = f.winner_buffer.data_ptr(), f._inputs[0].data_ptr()
    light = (C.c_float * 3)(-0.28, 0.19, -0.94)

    def guro():
        _capi.check(lib.crender_guro_illumination(f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(), light, size,
                                                  size, 0, size, st), "crender_guro_illumination")
    guro_us = round(_timed(stream, guro), 2)
    for persp in (False, True):
        for filt in ("nearest", "bilinear", "trilinear"):
            chain = filt == "trilinear"
            nflags = (_capi.NMAP_PERSPECTIVE if persp else 0) | (_capi.NMAP_BILINEAR if filt == "bilinear" else 0) | \
                (_capi.NMAP_CHAIN if chain else 0)

            def launch():
                _capi.check(lib.crender_nmap_shade(
                    win, d_tri, T, None, f._P, d_uv.data_ptr(), (d_map_chain if chain else d_map).data_ptr(), side, side, 1.0,
                    f.normals_buffer.data_ptr(), size, size, 0, size, nflags, st), "crender_nmap_shade")

            def launch_tex():
                if chain:
                    _capi.check(lib.crender_mip_shade(
                        win, d_tri, T, None, f._P, d_uv.data_ptr(), d_tex_chain.data_ptr(), side, side, None, None,
                        f.color_buffer.data_ptr(), size, size, 0, size, _capi.MIP_PERSPECTIVE if persp else 0, st),
                        "crender_mip_shade")
                else:
                    tflags = (_capi.TEX_PERSPECTIVE if persp else 0) | (_capi.TEX_BILINEAR if filt == "bilinear" else 0)
                    _capi.check(lib.crender_tex_shade(
                        win, d_tri, T, None, f._P, d_uv.data_ptr(), d_tex.data_ptr(), side, side, None, None,
                        f.color_buffer.data_ptr(), size, size, 0, size, tflags, st), "crender_tex_shade")
            us, tex_us = _timed(stream, launch), _timed(stream, launch_tex)
            # the planes' bytes: the winner word of every pixel, the normal read and written where a triangle won
            nbytes = 4 * npix + 24 * covered
            print(json.dumps({"scene": name, "T": T, "covered": round(covered / npix, 3),
                              "mode": ("perspective" if persp else "affine") + "_" + filt, "device_us": round(us, 2),
                              "texture_pass_us": round(tex_us, 2), "illumination_pass_us": guro_us,
                              "bytes_per_pixel": round(nbytes / npix, 2), "GB_per_s": round(nbytes / us / 1e3, 1)}), flush=True)

    d_height = torch.from_numpy(height).to(f.device)

    def make():
        _capi.check(lib.crender_nmap_from_height(d_height.data_ptr(), side, side, 1.0, 0, d_map.data_ptr(), st),
                    "crender_nmap_from_height")
    print(json.dumps({"scene": name, "mode": f"from_height_{side}x{side}", "device_us": round(_timed(stream, make), 2)}),
          flush=True)


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
            print(f"nmap_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
