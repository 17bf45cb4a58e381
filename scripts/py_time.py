"""Device time of the numpy filler (csrc/pyfill.hip): crender_py_draw between two HIP events, averaged
over repeated draws with CLEAR (each draw starts from the initial planes), for T-Rex at 1024^2 and 4096^2
in SimpleIterator and DepthIterator order; and the whole ``py.Renderer.render`` call on the host Buffers
(host wall time: colours, order, upload of inputs and planes, draw, Guro, download).
Also the device time of two triangles that cover most of a 4096^2 frame (a load the fragment walks
spread over every CU).  Prints one JSON line per case: python scripts/py_time.py"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cython3dmodelrenderer_amd import _capi, py, scenes  # noqa: E402
from cython3dmodelrenderer_amd.triangle_iterator import DepthIterator, SimpleIterator  # noqa: E402

REPS, WARMUP = 30, 3


class _Model:
    def __init__(self, tri, col, nrm):
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = tri, col, nrm


def main():
    lib = _capi.load()
    tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
    for size in (1024, 4096):
        for it in (SimpleIterator, DepthIterator):
            order = it.draw_order(_Model(tri, col, nrm))
            o = np.arange(len(tri)) if order is None else order
            d = [torch.from_numpy(np.ascontiguousarray(a[o])).cuda() for a in (tri, col, nrm)]
            z = torch.empty((size, size), dtype=torch.float32, device="cuda")
            c = torch.empty((size, size, 3), dtype=torch.uint8, device="cuda")
            n = torch.empty((size, size, 3), dtype=torch.float32, device="cuda")
            scratch = torch.empty(lib.crender_py_scratch_bytes(size, size, len(tri)), dtype=torch.uint8,
                                  device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            filler = py.pixel_buffer_filler.AdvancedPixelBufferFiller(size, size, fov=45)
            proj = (C.c_float * 4)(*filler._proj.tolist())
            stream = torch.cuda.current_stream()
            args = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(tri), proj, z.data_ptr(), c.data_ptr(),
                    n.data_ptr(), size, size, _capi.PY_CLEAR, scratch.data_ptr(), status.data_ptr(),
                    C.c_void_p(stream.cuda_stream))
            for _ in range(WARMUP):
                _capi.check(lib.crender_py_draw(*args), "crender_py_draw")
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(REPS):
                _capi.check(lib.crender_py_draw(*args), "crender_py_draw")
            b.record(stream)
            b.synchronize()
            assert int(status.item()) == 0
            dev_us = a.elapsed_time(b) * 1000.0 / REPS
            r = py.Renderer(filler, py.illumination.GuroIllumination([0, 0, 1]), it, size, size, use_tqdm=False)
            model = _Model(tri, col, nrm)
            r.render(model)
            t0 = time.perf_counter()
            for _ in range(REPS // 3):
                r.reset_buffers()
                r.render(model)
            call_ms = (time.perf_counter() - t0) * 1e3 / (REPS // 3)
            print(json.dumps({"scene": f"trex{size}", "T": int(len(tri)), "iterator": it.__name__,
                              "device_us_per_draw": round(dev_us, 1),
                              "renderer_render_ms_per_call": round(call_ms, 2)}), flush=True)
    time_large(lib)


def time_large(lib, size=4096):
    tri = np.float32([[[-0.9, -0.9, 1.0], [0.9, -0.8, 1.2], [0.0, 0.95, 0.9]],
                      [[-0.95, 0.9, 1.1], [0.9, 0.9, 0.95], [0.1, -0.9, 1.05]]])
    col = np.full((2, 3, 3), 128, np.float32)
    nrm = np.broadcast_to(np.float32([0.1, 0.2, -1]), (2, 3, 3)).copy()
    d = [torch.from_numpy(a).cuda() for a in (tri, col, nrm)]
    z = torch.empty((size, size), dtype=torch.float32, device="cuda")
    c = torch.empty((size, size, 3), dtype=torch.uint8, device="cuda")
    n = torch.empty((size, size, 3), dtype=torch.float32, device="cuda")
    scratch = torch.empty(lib.crender_py_scratch_bytes(size, size, 2), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    proj = (C.c_float * 4)(*py.pixel_buffer_filler.AdvancedPixelBufferFiller(size, size, fov=60)._proj.tolist())
    stream = torch.cuda.current_stream()
    args = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 2, proj, z.data_ptr(), c.data_ptr(), n.data_ptr(),
            size, size, _capi.PY_CLEAR, scratch.data_ptr(), status.data_ptr(), C.c_void_p(stream.cuda_stream))
    for _ in range(WARMUP):
        _capi.check(lib.crender_py_draw(*args), "crender_py_draw")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        _capi.check(lib.crender_py_draw(*args), "crender_py_draw")
    b.record(stream)
    b.synchronize()
    print(json.dumps({"scene": f"two_large_triangles{size}", "T": 2, "covered": round(float((z < 1e6).float().mean()), 3),
                      "device_us_per_draw": round(a.elapsed_time(b) * 1000.0 / REPS, 1)}), flush=True)


if __name__ == "__main__":
    main()
