"""Device time of the temporal resolve (csrc/temporal.hip, k_taa_resolve): crender_taa_resolve between two HIP events, mean
of 50 passes over the same frame, for T-Rex at 1024^2 and at 4096^2, in the three instances that matter: a static view (no
velocity plane), a velocity plane, and a velocity plane dilated by the z plane, each with the neighbourhood box.  The
history is the frame of the model turned by 2 degrees about y, the velocity plane crender_motion_vectors' against that
pose (its own time is a row of its own: the Renderer pays it every frame).  The pass only reads the frame, so every
repetition does the same work.

Next to them, in the same run, on the same frame: crender_wire_edge_aa (the other pass that reads the frame and writes a
colour plane of its own) and crender_guro_illumination (a plain pass over two planes).  Every row of the resolve carries its
ratios to them, and its bytes per pixel by the header's count with the bandwidth that would mean.  Every row is the mean of
three such measurements and carries their spread (largest minus smallest) as `spread_us`.  For reporting only: nothing is
gated on it.

Prints one JSON line per scene and case.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/taa_time.py [--scene trex1024]
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
# (name, a velocity plane, the z plane, bytes a pixel by include/crender_taa.h's count)
INSTANCES = (("static", False, False, 37.5), ("velocity", True, False, 46.5), ("dilated", True, True, 51.0))
CHILD_SECONDS = 300


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
    prev = _rotated(tri, 2.0)
    f.render_arrays(prev, col, nrm, clear=True)
    history = f.temporal_resolve(None)                 # the frame of the pose before, copied
    f.render_arrays(*[torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)], clear=True)
    velocity = f.motion_vectors(prev)                  # settles the frame; the direct calls below repeat the passes
    out = torch.empty_like(history)
    covered = int((f.get_winner_tensor() >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    T = int(tri.shape[0])
    d_prev = torch.from_numpy(prev).to(f.device)
    shaded = torch.empty_like(f.color_buffer)          # the light pass writes its colour plane: a copy takes it
    light = (C.c_float * 3)(0.3, -0.2, 1.0)

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "mode": mode, "device_us": round(us, 2),
             "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    def guro():
        _capi.check(lib.crender_guro_illumination(shaded.data_ptr(), f.normals_buffer.data_ptr(), light, size, size, 0, size, st),
                    "crender_guro_illumination")
    shaded.copy_(f.color_buffer)
    guro_us = row("guro_illumination", _timed(stream, guro))

    def edge_aa():
        _capi.check(lib.crender_wire_edge_aa(
            f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, None, out.data_ptr(),
            f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_wire_edge_aa")
    aa_us = row("edge_aa", _timed(stream, edge_aa))

    def vectors():
        _capi.check(lib.crender_motion_vectors(
            f.winner_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, d_prev.data_ptr(), 1.0, velocity.data_ptr(), size,
            size, 0, size, 0, st), "crender_motion_vectors")
    row("motion_vectors", _timed(stream, vectors))
    for mode, moving, dilate, nbytes in INSTANCES:
        def resolve():
            _capi.check(lib.crender_taa_resolve(
                f.color_buffer.data_ptr(), history.data_ptr(), velocity.data_ptr() if moving else None,
                f.z_buffer.data_ptr() if dilate else None, 0.1, out.data_ptr(), size, size, 0, size, 0, st), "crender_taa_resolve")
        us, spread = _timed(stream, resolve)
        row(f"taa_resolve_{mode}", (us, spread), bytes_per_pixel=nbytes, gb_per_s=round(nbytes * npix / us / 1e3, 1),
            vs_edge_aa=round(us / aa_us, 3), vs_guro=round(us / guro_us, 3))


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
            print(f"taa_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
