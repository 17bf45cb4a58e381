"""Device time of the depth-of-field pass (csrc/dof.hip, k_dof_blur): crender_dof_blur between two HIP events, mean
of 50 passes over the same frame, for T-Rex at 1024^2 and at 4096^2, at max_radius 4, 8 and 12, in two cases, both with
an aperture of four times max_radius: FOCUSED — the focus on the median view depth of the model with a band that holds
the whole model, so that every tile that sees the model alone finds nothing blurred around it and copies (`copy_tiles`
is their share of the tiles; the background, which is at infinity, blurs at the clamp whatever the band, and the
tiles that see it walk their full window) — and BLURRED — no band: the background and most of the model sit at the
clamp and every tile walks its full window.  The pass only reads the frame, so every repetition does the same work.

Next to it, in the same run, on the same frame: crender_ao_shade with 64 taps at the same pixel radius (the other
neighbourhood pass staged in LDS: one word a pixel and 64 taps, against five words and up to (2 R + 1)^2 taps), and
crender_wire_edge_aa (the other pass that writes a plane of its own); every row of the new pass carries its ratios to
them as `vs_ao64` and `vs_edge_aa`.  Every row is the mean of three such measurements and carries their spread (largest
minus smallest) as `spread_us`.  For reporting only: nothing is gated on it.

Prints one JSON line per scene, radius and case.  Run without arguments it measures each scene in a child process of its
own under ``timeout`` and stops at the first one that fails:

  python scripts/dof_time.py [--scene trex1024]
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
RADII = (4, 8, 12)
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
    from cython3dmodelrenderer_amd import _capi, ambient_occlusion, scenes
    from cython3dmodelrenderer_amd.depth_of_field import view_depth
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size = SCENES[name]
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    f = AdvancedPixelBufferFiller(size, size, fov=45.0, track_winner=True)
    dev = [torch.from_numpy(a).to(f.device) for a in (tri, col, nrm)]
    f.render_arrays(*dev, clear=True)
    out = f.edge_aa()                                  # settles the frame; the direct calls below repeat the passes
    winner = f.get_winner_tensor()
    zv = view_depth(f._P, f.get_z_tensor())[winner >= 0]
    focus = float(zv.median())
    whole = float(max(zv.max() - focus, focus - zv.min())) * 1.01      # a band that holds the whole model
    covered = int((winner >= 0).sum())
    npix = size * size
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    T = int(tri.shape[0])
    shaded = torch.empty_like(f.color_buffer)          # the occlusion pass writes its colour plane: a copy takes it

    def row(mode, timed, **more):
        us, spread = timed
        r = {"scene": name, "T": T, "covered": round(covered / npix, 3), "mode": mode, "device_us": round(us, 2),
             "spread_us": round(spread, 2), **more}
        print(json.dumps(r), flush=True)
        return us

    def edge_aa():
        _capi.check(lib.crender_wire_edge_aa(
            f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P, None, out.data_ptr(),
            f.color_buffer.data_ptr(), size, size, 0, size, 0, st), "crender_wire_edge_aa")
    edge_us = row("edge_aa_all", _timed(stream, edge_aa))
    for R in RADII:
        table = ambient_occlusion.taps(R, 64)
        taps2 = (C.c_int8 * (2 * len(table)))(*[v for pair in table for v in pair])

        def ao():
            _capi.check(lib.crender_ao_shade(
                f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), f._inputs[0].data_ptr(), T, None, f._P,
                f.normals_buffer.data_ptr(), taps2, len(table), R, 0.05, 0.1, 2.0, 0.0, shaded.data_ptr(), size, size, 0, size,
                _capi.AO_ROTATE, st), "crender_ao_shade")
        shaded.copy_(f.color_buffer)
        ao_us = row(f"ao_64_taps_r{R}", _timed(stream, ao))
        # focused: everything the model shows is within the band, so a tile copies iff its 32 x 32 pixels and their halo
        # of R hold no background (what lies off the frame does not count)
        background = (winner < 0).to(torch.float32)[None, None]
        seen = torch.nn.functional.max_pool2d(background, 32 + 2 * R, stride=32, padding=R, ceil_mode=True)
        copy_tiles = round(float((seen == 0).sum()) / seen.numel(), 3)
        for case, kw in (("focused", dict(band=whole, aperture=4.0 * R, copy_tiles=copy_tiles)),
                         ("blurred", dict(band=0.0, aperture=4.0 * R, copy_tiles=0.0))):
            def blur():
                _capi.check(lib.crender_dof_blur(
                    f.winner_buffer.data_ptr(), f.z_buffer.data_ptr(), None, T, None, f._P, f.color_buffer.data_ptr(), focus,
                    kw["band"], kw["aperture"], R, out.data_ptr(), size, size, 0, size, 0, st), "crender_dof_blur")
            us, spread = _timed(stream, blur)
            row(f"dof_{case}_r{R}", (us, spread), copy_tiles=kw["copy_tiles"], vs_ao64=round(us / ao_us, 2), vs_edge_aa=round(us / edge_us, 2))


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
            print(f"dof_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
