"""Device time of the wireframe filler (csrc/wireframe.hip): crender_wire_draw between two HIP events,
averaged over repeated draws onto the same planes, for T-Rex at 1024^2 and the bunny at 4096^2 (each
fitted as Renderer.render(normalize_model=True) fits it), in every mode; and the whole
``render_arrays`` call from device-resident inputs (host wall time, with its one synchronisation).
Prints one JSON line per mesh and mode: python scripts/wire_time.py"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from cython3dmodelrenderer_amd import _capi, scenes  # noqa: E402
from cython3dmodelrenderer_amd.pixel_buffer_filler import EdgeOnlyPixelBufferFiller, LineBresenham  # noqa: E402

REPS, WARMUP = 50, 5


def main():
    lib = _capi.load()
    rows = []
    for name, fixture, size in (("trex1024", "trex_inputs.npz", 1024), ("bunny4096", "bunny_inputs.npz", 4096)):
        tri, col, _ = scenes.load_fixture(fixture)
        fitted = scenes.fit_soup_to_frame(tri, size, size)
        d_tri = torch.from_numpy(fitted).cuda()
        d_col = torch.from_numpy(col).cuda()
        for edges in (True, False):
            for forced in (False, True):
                f = EdgeOnlyPixelBufferFiller(LineBresenham(), (255.0, 255.0, 255.0), draw_edges=edges,
                                              force_triangle_colors=forced, h=size, w=size)
                f.render_arrays(d_tri, d_col)                   # allocates the planes (and the key plane)
                flags = (0 if edges else _capi.WIRE_DOTS) | (_capi.WIRE_FORCE_COLORS if forced else 0)
                line = (C.c_float * 3)(255.0, 255.0, 255.0)
                args = (d_tri.data_ptr(), d_col.data_ptr() if forced else None, d_tri.shape[0], line,
                        f.z_buffer.data_ptr(), f.color_buffer.data_ptr(), f.normals_buffer.data_ptr(),
                        f._key.data_ptr() if forced else None, size, size, flags, f._status.data_ptr())
                stream = torch.cuda.current_stream()
                for _ in range(WARMUP):
                    _capi.check(lib.crender_wire_draw(*args, C.c_void_p(stream.cuda_stream)), "crender_wire_draw")
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(REPS):
                    _capi.check(lib.crender_wire_draw(*args, C.c_void_p(stream.cuda_stream)), "crender_wire_draw")
                b.record(stream)
                b.synchronize()
                dev_us = a.elapsed_time(b) * 1000.0 / REPS
                t0 = time.perf_counter()
                for _ in range(REPS):
                    f.render_arrays(d_tri, d_col)
                call_us = (time.perf_counter() - t0) * 1e6 / REPS
                row = {"scene": name, "T": int(tri.shape[0]), "mode": ("edges" if edges else "dots")
                       + ("_forced" if forced else "_line"), "device_us_per_draw": round(dev_us, 2),
                       "render_arrays_us_per_call": round(call_us, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
