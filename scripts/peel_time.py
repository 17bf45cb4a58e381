"""Device time of transparency (csrc/peel.hip: k_peel_seed, k_peel_cover, k_peel_resolve, k_peel_blend): one
crender_peel_next (the layer behind the frame's own), one crender_peel_blend (a middle layer: shaded from the model, read
and add), and ``transparency_pass`` at 2, 4 and 8 layers, each between two HIP events, mean of 20 calls over the same
frame, for T-Rex at 1024^2 and the bunny at 4096^2, alpha 0.5 everywhere.  Every pass only reads the frame, so every
repetition does the same work.

Next to them, in the same run, on the same scene: ``lowlevel.raster_atomic`` on the projected triangles — the same walk
(a wavefront per triangle, 8 x 8 steps, a 64-bit atomicMin) without the 8-byte read of the previous key, and a resolve
that stores colours and normals as well — and the frame's own ``render_arrays`` + settle.  Every row of the new entries
carries its ratio to the first as `vs_raster_atomic` and to the second as `vs_frame`.  Every row is the mean of three
such measurements and carries their spread (largest minus smallest) as `spread_us`.  For reporting only: nothing is gated
on it.

Prints one JSON line per scene and case.  Run without arguments it measures each scene in a child process of its own
under ``timeout`` and stops at the first one that fails:

  python scripts/peel_time.py [--scene trex1024]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARMUP, ROUNDS = 20, 3, 3
SCENES = ("trex1024", "bunny4096")
LAYERS = (2, 4, 8)
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


def measure(name):
    import torch
    from cython3dmodelrenderer_amd import _capi, lowlevel, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    tri, col, nrm, (H, W), fov = scenes.scene(name)
    f = AdvancedPixelBufferFiller(H, W, fov=fov, track_winner=True)
    dev = [torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)]
    T = int(tri.shape[0])
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "mode": mode, "device_us": round(us, 2), "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    def frame():
        f.render_arrays(*dev, clear=True)
        f.synchronize()
    frame_us = row("frame_render_arrays_settle", _timed(stream, frame))
    # the same walk without the previous key: the atomic path on the projected triangles, into planes of its own
    P = lowlevel.projection_matrix(fov, 0.1, 1000.0, H, W)
    proj = lowlevel.project(dev[0], P, W, H)
    fb = lowlevel.FrameBuffers(H, W, device=f.device)
    keys = lowlevel.raster_atomic(proj, dev[1], dev[2], fb, clear=True)
    atomic_us = row("raster_atomic", _timed(stream, lambda: lowlevel.raster_atomic(proj, dev[1], dev[2], fb, clear=True, keys=keys)))
    # the entries on the frame's own planes and resident inputs
    winners, zs = f.peel_layers(3)                      # settles the frame, allocates the scratch
    covered = [round(float((winners[k] >= 0).sum()) / (H * W), 3) for k in range(3)]
    itri, icol, inrm = f._inputs
    pos_of = None if f._order is None else f._order[1].data_ptr()
    scratch, trans, _, _ = f._peel_scratch
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=f.device)
    alpha = torch.full((T,), 0.5, dtype=torch.float32, device=f.device)
    w1, z1 = torch.empty_like(winners[0]), torch.empty_like(zs[0])
    ratios = lambda us: dict(vs_raster_atomic=round(us / atomic_us, 2), vs_frame=round(us / frame_us, 2))     # noqa: E731

    def peel():
        _capi.check(lib.crender_peel_next(winners[0].data_ptr(), zs[0].data_ptr(), itri.data_ptr(), T, pos_of, f._P,
                                          inrm.data_ptr(), scratch.data_ptr(), w1.data_ptr(), z1.data_ptr(), H, W, 0, H, 0, st),
                    "crender_peel_next")
    timed = _timed(stream, peel)
    row("peel_next_layer_1", timed, covered_layers=covered, **ratios(timed[0]))
    ground = (C.c_float * 3)(0.0, 0.0, 0.0)
    trans.fill_(0.5)

    def blend():
        _capi.check(lib.crender_peel_blend(winners[1].data_ptr(), itri.data_ptr(), T, pos_of, f._P, icol.data_ptr(),
                                           inrm.data_ptr(), alpha.data_ptr(), None, None, ground, trans.data_ptr(),
                                           out.data_ptr(), H, W, 0, H, 0, st), "crender_peel_blend")
    timed = _timed(stream, blend)
    row("peel_blend_layer_1", timed, **ratios(timed[0]))
    for n in LAYERS:
        timed = _timed(stream, lambda: f.transparency_pass(alpha, layers=n))
        row(f"transparency_pass_{n}_layers", timed, **ratios(timed[0]))


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
            print(f"peel_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
