"""Device time of the texture pass (csrc/texture.hip, csrc/texmip.hip, csrc/texaniso.hip): crender_tex_shade,
crender_mip_shade and crender_aniso_shade between two HIP events, mean of 50 passes over the same frame, for T-Rex
at 256^2 (where most pixels are minified), 1024^2 and 4096^2 under a random 709 x 709 texture and for the receding
floor of tests/aniso_ref.py at 1024^2 under a random 2048 x 2048 one (where anisotropy bites), in the four modes of
the first, the two of the second (trilinear rows carry the bilinear time of the same frame and run as
`bilinear_us`) and the second's at max_aniso 2, 4 and 16 (with the trilinear time as `trilinear_us` and the mean
sample count over covered pixels, from the host model, as `mean_N`, and the share that takes one sample as
`one_sample`), with and without the fused light; next to
them, the existing illumination pass alone (crender_guro_illumination) on the same frames — the figure the fused
light has to beat is pass + illumination — and crender_mip_build of the texture.

Prints one JSON line per scene and mode.  Run without arguments it measures each scene in a child process of its
own under ``timeout`` and stops at the first one that fails:

  python scripts/tex_time.py [--scene trex1024]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))        # the host model: aniso_ref (mean_N, the floor scene)

REPS, WARMUP = 50, 5
SCENES = {"trex256": (256, 709), "trex1024": (1024, 709), "trex4096": (4096, 709), "floor1024": (1024, 2048)}
ANISO = (2, 4, 16)
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
    import aniso_ref
    lib = _capi.load()
    size, side = SCENES[name]
    if name.startswith("floor"):
        tri, col, nrm, uv = aniso_ref.floor_scene()
    else:
        tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
        with np.load(os.path.join(scenes.GOLDEN_DIR, "trex_uv.npz")) as z:
            uv = np.ascontiguousarray(z["uv"][z["faces_uv"]], dtype=np.float32)
    tex = np.random.default_rng(1).integers(0, 256, (side, side, 3), dtype=np.uint8)
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    f.bind_texture(uv, tex, mipmaps=True)
    f.render_arrays(tri, col, nrm, clear=True)
    f.texture_pass()                                   # settles the frame; the direct calls below repeat the pass
    d_uv, d_tex = f._texture
    d_chain = f._mip[0]
    assert f._order is None                            # (below 2^18 triangles the inputs stay in the caller's order)
    winner = f.get_winner_tensor().cpu().numpy()
    covered = int((winner >= 0).sum())
    P = f.proj_mat
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    light = (C.c_float * 3)(-0.28, 0.19, -0.94)
    rows = []
    mean_n = {}                  # (perspective, A) -> (mean sample count, share of N == 1) over covered pixels, host model

    def row(mode, us, nbytes, **more):
        r = {"scene": name, "T": int(tri.shape[0]), "covered": round(covered / npix, 3), "mode": mode,
             "device_us": round(us, 2), "bytes_per_pixel": round(nbytes / npix, 2),
             "GB_per_s": round(nbytes / us / 1e3, 1), **more}
        rows.append(r)
        print(json.dumps(r), flush=True)
        return r

    for with_light in (False, True):
        for persp in (False, True):
            for bilinear in (False, True):
                flags = (_capi.TEX_PERSPECTIVE if persp else 0) | (_capi.TEX_BILINEAR if bilinear else 0)

                def launch():
                    _capi.check(lib.crender_tex_shade(
                        f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), tri.shape[0], None, f._P, d_uv.data_ptr(),
                        d_tex.data_ptr(), side, side, f.normals_buffer.data_ptr() if with_light else None,
                        light if with_light else None, f.color_buffer.data_ptr(), size, size, 0, size, flags, st),
                        "crender_tex_shade")
                # the planes' bytes: the winner word of every pixel and the colour stored where a triangle won; with a
                # light the normal of every pixel too, and the background's colour read and written
                nbytes = 4 * npix + 12 * covered
                if with_light:
                    nbytes += 12 * npix + 24 * (npix - covered)
                mode = ("perspective" if persp else "affine") + ("_bilinear" if bilinear else "_nearest") + \
                    ("_light" if with_light else "")
                bilinear_us = row(mode, _timed(stream, launch), nbytes)["device_us"]

            def launch_mip():
                _capi.check(lib.crender_mip_shade(
                    f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), tri.shape[0], None, f._P, d_uv.data_ptr(),
                    d_chain.data_ptr(), side, side, f.normals_buffer.data_ptr() if with_light else None,
                    light if with_light else None, f.color_buffer.data_ptr(), size, size, 0, size,
                    _capi.MIP_PERSPECTIVE if persp else 0, st), "crender_mip_shade")
            mode = ("perspective" if persp else "affine") + "_trilinear" + ("_light" if with_light else "")
            trilinear_us = row(mode, _timed(stream, launch_mip), nbytes, bilinear_us=bilinear_us)["device_us"]

            for A in ANISO:
                def launch_aniso():
                    _capi.check(lib.crender_aniso_shade(
                        f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), tri.shape[0], None, f._P, d_uv.data_ptr(),
                        d_chain.data_ptr(), side, side, f.normals_buffer.data_ptr() if with_light else None,
                        light if with_light else None, f.color_buffer.data_ptr(), size, size, 0, size,
                        _capi.MIP_PERSPECTIVE if persp else 0, A, st), "crender_aniso_shade")
                if (persp, A) not in mean_n:
                    N = aniso_ref.pixel_footprints(winner, tri, P, uv, side, side, persp, A)[6]
                    mean_n[persp, A] = (round(float(N.mean()), 3), round(float((N == 1).mean()), 4))
                mode = ("perspective" if persp else "affine") + f"_aniso{A}" + ("_light" if with_light else "")
                row(mode, _timed(stream, launch_aniso), nbytes, trilinear_us=trilinear_us, mean_N=mean_n[persp, A][0],
                    one_sample=mean_n[persp, A][1])

    def guro():
        _capi.check(lib.crender_guro_illumination(f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(), light, size,
                                                  size, 0, size, st), "crender_guro_illumination")
    row("illumination_pass_alone", _timed(stream, guro), 36 * npix)

    def build():
        _capi.check(lib.crender_mip_build(d_tex.data_ptr(), side, side, d_chain.data_ptr(), st), "crender_mip_build")
    us = _timed(stream, build)
    print(json.dumps({"scene": name, "mode": f"mip_build_{side}x{side}", "levels": len(f.mip_levels()),
                      "chain_bytes": int(d_chain.numel()), "device_us": round(us, 2)}), flush=True)
    return rows


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
            print(f"tex_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
