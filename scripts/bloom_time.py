"""Device time of bloom and tone mapping (csrc/bloom.hip, k_bloom_rows and k_bloom_finish): crender_bloom — both
launches — between two HIP events, mean of 50 calls over the same image, for T-Rex under a Phong light with clamp=inf
(so that its highlights exceed 255) at 1024^2 and at 4096^2, at radius 4, 12 and 32, in two cases: DARK — a threshold
above every pixel: nothing is bright, every wavefront of the first launch and every tile of the second skips its walk,
and the pass is two sweeps over the image — and LIT — the threshold at the median of the covered pixels' largest
channel, so that half of the model glows and every tile within its reach walks all of its 2 (2 R + 1) taps
(`bright` is the share of bright pixels).  The pass only reads the image, so every repetition does the same work.

Next to it, in the same run, on the same frame: crender_guro_illumination (a sweep over two planes: what a pass costs
that only streams) and crender_dof_blur at max_radius 4 and 12 with everything at the clamp (the gather over
(2 R + 1)^2 taps that the separable walk stands against); every row of the new pass carries its ratio to the former as
`vs_guro` and, at 4 and 12, to the latter as `vs_dof`.  Every row is the mean of three such measurements and carries
their spread (largest minus smallest) as `spread_us`.  For reporting only: nothing is gated on it.

Prints one JSON line per scene, radius and case.  Run without arguments it measures each scene in a child process of its
own under ``timeout`` and stops at the first one that fails:

  python scripts/bloom_time.py [--scene trex1024]
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
RADII = (4, 12, 32)
CHILD_SECONDS = 300
LIGHTS = [dict(position=(0.1, -0.1, 1.5), diffuse=0.8, specular=0.9)]


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
    from cython3dmodelrenderer_amd import _capi, bloom, scenes
    from cython3dmodelrenderer_amd.depth_of_field import view_depth
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    dev = [torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)]
    f.render_arrays(*dev, clear=True)
    f.phong_pass(LIGHTS, ambient=0.15, shininess=8, clamp=float("inf"))
    image = f.get_color_tensor()                       # settles the frame; the direct calls below repeat the passes
    winner = f.get_winner_tensor()
    largest = image.max(dim=2).values
    top = float(largest.max())
    median = float(largest[winner >= 0].median())
    covered = int((winner >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    T = int(tri.shape[0])
    out, scratch, shaded = torch.empty_like(image), torch.empty_like(image), image.clone()

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "above_255": round(float((largest > 255).sum()) / npix, 4),
             "mode": mode, "device_us": round(us, 2), "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    light = (C.c_float * 3)(0.2873, -0.1915, -0.9386)

    def guro():                                        # (shades its plane again and again: the time does not depend on the values)
        _capi.check(lib.crender_guro_illumination(shaded.data_ptr(), f.normals_buffer.data_ptr(), light, size, size, 0, size, st),
                    "crender_guro_illumination")
    guro_us = row("guro_illumination", _timed(stream, guro))
    zv = view_depth(f._P, f.get_z_tensor())[winner >= 0]
    focus = float(zv.median())
    dof_us = {}
    for R in (4, 12):
        def blur():
            _capi.check(lib.crender_dof_blur(
                f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), None, T, None, f._P, image.data_ptr(), focus, 0.0, 4.0 * R, R,
                out.data_ptr(), size, size, 0, size, 0, st), "crender_dof_blur")
        dof_us[R] = row(f"dof_blurred_r{R}", _timed(stream, blur))
    for R in RADII:
        for case, threshold in (("dark", top + 1.0), ("lit", median)):
            call = bloom.arguments(threshold=threshold, radius=R, tonemap="reinhard")

            w = (C.c_float * (R + 1))(*call.weights.tolist())

            def glow():
                _capi.check(lib.crender_bloom(image.data_ptr(), call.threshold, w, R, call.intensity, call.exposure,
                                              call.inv_white2, call.clamp, scratch.data_ptr(), out.data_ptr(), size, size, 0,
                                              size, call.flags, st), "crender_bloom")
            us, spread = _timed(stream, glow)
            more = {"bright": round(float((largest > threshold).sum()) / npix, 3), "vs_guro": round(us / guro_us, 2),
                    "ps_per_pixel_tap": round(us * 1e6 / (npix * 2 * (2 * R + 1)), 2)}
            if R in dof_us:
                more["vs_dof"] = round(us / dof_us[R], 3)
            row(f"bloom_{case}_r{R}", (us, spread), **more)


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
            print(f"bloom_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
