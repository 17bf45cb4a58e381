"""Device time of the supersampling resolve (csrc/resolve.hip): crender_ssaa_resolve between two HIP events, mean of
50 calls on the same planes, for T-Rex rendered at 2048^2 and resolved to 1024^2 (s = 2), at 4096^2 to 1024^2 (s = 4)
and at 8192^2 to 2048^2 (s = 4): the plain resolve, the resolve with the fused light, and the resolve with the light,
the uint8 cast and the row flip.  In the same run, the unfused chain they replace — crender_guro_illumination over the
source, the plain resolve, crender_present_u8 of the result — whose first step is also the yardstick: a plain
streaming kernel of this project over the same source frame.

`GB_per_s` is the EFFECTIVE bandwidth: the contract's bytes — 12 s^2 read per output pixel (24 s^2 with the light)
plus 12 or 3 written; 36 per source pixel for the illumination pass; 12 read and 3 written per pixel for the
presentation — divided by the time.

Prints one JSON line per scene and mode, then one line per scene with the two ratios.  Run without arguments it
measures each scene in a child process of its own under ``timeout`` and stops at the first one that fails:

  python scripts/ssaa_time.py [--scene trex4096]
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
SCENES = {"trex2048": (2048, 2), "trex4096": (4096, 4), "trex8192": (8192, 4)}      # source size, factor
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
    import torch
    from cython3dmodelrenderer_amd import _capi, scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    lib = _capi.load()
    size, s = SCENES[name]
    out_size = size // s
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    f = AdvancedPixelBufferFiller(size, size, fov=45.0)
    f.render_arrays(tri, col, nrm, clear=True)
    f.synchronize()                                    # the frame is settled; the direct calls below read its planes
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    light = (C.c_float * 3)(-0.28, 0.19, -0.94)
    out32 = torch.empty((out_size, out_size, 3), dtype=torch.float32, device="cuda:0")
    out8 = torch.empty((out_size, out_size, 3), dtype=torch.uint8, device="cuda:0")
    src_px, out_px = size * size, out_size * out_size
    times = {}

    def row(mode, us, nbytes):
        times[mode] = (us, nbytes / us / 1e3)
        print(json.dumps({"scene": name, "source": f"{size}x{size}", "s": s, "mode": mode, "device_us": round(us, 2),
                          "bytes_per_output_pixel": round(nbytes / out_px, 2), "GB_per_s": round(nbytes / us / 1e3, 1)}),
              flush=True)

    def resolve(with_light, out, flags):
        def launch():
            _capi.check(lib.crender_ssaa_resolve(
                f.color_buffer.data_ptr(), f.normals_buffer.data_ptr() if with_light else None,
                light if with_light else None, size, size, s, 0, out_size, out.data_ptr(), flags, st),
                "crender_ssaa_resolve")
        return launch

    row("resolve", _timed(stream, resolve(False, out32, 0)), (12 * s * s + 12) * out_px)
    row("resolve_light", _timed(stream, resolve(True, out32, 0)), (24 * s * s + 12) * out_px)
    row("resolve_light_u8_flip", _timed(stream, resolve(True, out8, _capi.SSAA_U8 | _capi.SSAA_FLIP)),
        (24 * s * s + 3) * out_px)

    def present():
        _capi.check(lib.crender_present_u8(out32.data_ptr(), out8.data_ptr(), out_size, out_size, 1, st),
                    "crender_present_u8")
    row("present_u8_alone", _timed(stream, present), 15 * out_px)

    # last: the pass shades the source colour plane in place, every call
    def guro():
        _capi.check(lib.crender_guro_illumination(f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(), light, size,
                                                  size, 0, size, st), "crender_guro_illumination")
    row("illumination_pass_alone", _timed(stream, guro), 36 * src_px)

    chain = times["illumination_pass_alone"][0] + times["resolve"][0] + times["present_u8_alone"][0]
    print(json.dumps({"scene": name, "unfused_chain_us": round(chain, 2),
                      "fused_us": round(times["resolve_light_u8_flip"][0], 2),
                      "chain_over_fused": round(chain / times["resolve_light_u8_flip"][0], 2),
                      "resolve_bandwidth_over_illumination_pass": round(times["resolve"][1] /
                                                                        times["illumination_pass_alone"][1], 2)}),
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
            print(f"ssaa_time: scene {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
