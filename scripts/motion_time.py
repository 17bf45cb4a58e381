"""Device time of the motion passes (csrc/motion.hip, k_motion_vectors and k_motion_blur): crender_motion_vectors and
crender_motion_blur between two HIP events, mean of 50 passes over the same frame, for T-Rex at 1024^2 and at 4096^2, at
max_radius 4, 8 and 12 and 8, 16 and 32 taps.  The previous pose is the model rotated about y around the mean of its
corners by an angle found by bisection, so that the largest half velocity of the frame reaches max_radius (`largest_l`
in every row; `walk_tiles` is the share of the tiles whose dominant pixel moves by more than a pixel: the others copy).
The passes only read the frame, so every repetition does the same work.

Next to them, in the same run, on the same frame: crender_shadow_shade with one tap against the frame itself as the
light's (the pass that does the vectors' gathers: the winner's triangle and a second set of corners, 72 B per distinct
winner), crender_dof_blur at the same radius with every pixel at the clamp (the other five-plane pass staged in LDS:
(2 R + 1)^2 taps against at most 32), and crender_guro_illumination (a plain pass over two planes).  Every row of the new
passes carries its ratios to them, and the blur's rows the picoseconds per pixel and tap.  Every row is the mean of three
such measurements and carries their spread (largest minus smallest) as `spread_us`.  For reporting only: nothing is gated
on it.

Prints one JSON line per scene and case.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/motion_time.py [--scene trex1024]
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
RADII = (4, 8, 12)
TAPS = (8, 16, 32)
CHILD_SECONDS = 400


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


def _rotated(tri, degrees):
    """`tri` rotated about y by `degrees` around the float32 mean of its corners."""
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]).astype(np.float32)
    c = tri.reshape(-1, 3).mean(0, dtype=np.float32)
    return np.ascontiguousarray(((tri.reshape(-1, 3) - c) @ R.T + c).reshape(tri.shape).astype(np.float32))


def measure(name):
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    dev = [torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)]
    f.render_arrays(*dev, clear=True)
    out = f.edge_aa()                                  # settles the frame; the direct calls below repeat the passes
    winner = f.get_winner_tensor()
    covered = int((winner >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    T = int(tri.shape[0])
    shaded = torch.empty_like(f.color_buffer)          # the shadow and light passes write their colour plane: a copy takes it
    velocity = torch.empty((size, size, 2), dtype=torch.float32, device=f.device)
    light = (C.c_float * 3)(0.3, -0.2, 1.0)

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "mode": mode, "device_us": round(us, 2),
             "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    def vectors(prev):
        _capi.check(lib.crender_motion_vectors(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, prev.data_ptr(), 1.0, velocity.data_ptr(), size,
            size, 0, size, 0, st), "crender_motion_vectors")

    def largest_half(prev):
        vectors(prev)
        return float(velocity.square().sum(2).sqrt().max()) / 2

    def guro():
        _capi.check(lib.crender_guro_illumination(shaded.data_ptr(), f.normals_buffer.data_ptr(), light, size, size, 0, size, st),
                    "crender_guro_illumination")
    shaded.copy_(f.color_buffer)
    guro_us = row("guro_illumination", _timed(stream, guro))

    def shadow():
        # the frame itself as the light's: the vectors' gathers, one tap into its own z plane
        _capi.check(lib.crender_shadow_shade(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, f._inputs[0].data_ptr(), f._P,
            f.z_buffer.data_ptr(), None, size, size, 1e-3, 0.25, 1, shaded.data_ptr(), size, size, 0, size, 0, st),
            "crender_shadow_shade")
    shaded.copy_(f.color_buffer)
    shadow_us = row("shadow_1_tap", _timed(stream, shadow))
    for R in RADII:
        # the angle at which the largest half velocity reaches R: it grows with the angle over this range
        lo, hi = 0.0, 45.0
        for _ in range(24):
            mid = (lo + hi) / 2
            if largest_half(torch.from_numpy(_rotated(tri, mid)).to(f.device)) < R:
                lo = mid
            else:
                hi = mid
        prev = torch.from_numpy(_rotated(tri, hi)).to(f.device)
        top = largest_half(prev)
        us, spread = _timed(stream, lambda: vectors(prev))
        row(f"motion_vectors_r{R}", (us, spread), degrees=round(hi, 3), largest_l=round(top, 3),
            vs_shadow=round(us / shadow_us, 2), vs_guro=round(us / guro_us, 2))
        vectors(prev)
        half = velocity.square().sum(2).sqrt() / 2
        seen = torch.nn.functional.max_pool2d(half[None, None], 32 + 2 * R, stride=32, padding=R, ceil_mode=True)
        walk_tiles = round(float((seen > 0.5).sum()) / seen.numel(), 3)

        def dof():
            # every pixel at the clamp: the full window of (2 R + 1)^2 taps
            _capi.check(lib.crender_dof_blur(
                f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), None, T, None, f._P, f.color_buffer.data_ptr(), 1.0, 0.0,
                1e6, R, out.data_ptr(), size, size, 0, size, 0, st), "crender_dof_blur")
        dof_us = row(f"dof_blurred_r{R}", _timed(stream, dof))
        for N in TAPS:
            def blur():
                _capi.check(lib.crender_motion_blur(
                    f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), None, T, None, f._P, f.color_buffer.data_ptr(),
                    velocity.data_ptr(), R, N, 0.02, out.data_ptr(), size, size, 0, size, 0, st), "crender_motion_blur")
            us, spread = _timed(stream, blur)
            row(f"motion_blur_r{R}_taps{N}", (us, spread), walk_tiles=walk_tiles, largest_l=round(top, 3),
                ps_per_pixel_tap_walked=round(us * 1e6 / (npix * walk_tiles * N), 2) if walk_tiles else None,
                vs_dof=round(us / dof_us, 3), vs_guro=round(us / guro_us, 2))


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
            print(f"motion_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
