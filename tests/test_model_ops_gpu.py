"""The kernels of csrc/model_ops.hip through their C entries, bit for bit (a NaN for a NaN) against the numpy models of
tests/model_ref.py, which tests/test_model_ops_cpu.py pins against numpy and the host ``Model``: hand-built operands
at the edges — specials, empty and one-element inputs, sizes either side of every window — and one size past
2^20 items per entry, at which its grid-stride loop takes a second trip (4 096 blocks of 256 threads; 1 024 for the
span).  Then ``DeviceModel`` against the host ``Model`` in seeded sessions that draw the argument's kind.

What the file was shown to catch: library builds with one arithmetic change each (never an index, a bound or a
pointer), the first test of this file that failed on each, and whether the suite before this file failed (*):
  k_guro without ``0.0f +``                 test_guro_on_painted_planes_strips_and_lights[33-67]: -0 for +0, 87 elements (*)
  k_present_u8 with ``<=`` at 2^31          test_present_u8_on_the_value_table[1-1]: 255 for 0
  k_model_shift ignoring in_double          test_model_shift[1]: 3 of 3 elements (*)
  k_model_scale ignoring in_double          test_model_scale_both_entries[1]: 1 of 3 elements
  k_model_mean adding its 32 rows pairwise  test_model_stats[34]: mean, 2 of 3 elements (*)
  k_model_mean starting from the first row  test_model_stats[1]: all -0, mean -0 for +0 (the kernel before this file)
  k_model_max_span without the NaN branch   test_model_stats[1]: span 0 for NaN
  dot3_f32 as a plain float32 sum           test_vertex_normals_on_the_edge_meshes: fan of 200, 80 of 600 face normals (*)
  the de-duplication as ``> 1.0f``          test_vertex_normals_on_the_edge_meshes: coplanar fan, 126 of 192 taken bytes (*)
  k_model_rotate grouped from the right     test_model_rotate[1]: 0 for 2.2090495
  k_tile_order_keys, one trip only          test_tile_order_keys[1048640]: the last 64 keys unwritten
  k_model_gather, one trip only             test_model_gather[349526-1]: the last 6 elements unwritten
(k_model_texture_colors clamping the row to ``th``: the row only forms the address, so there is no such change.)"""
import ctypes as C

import numpy as np
import pytest

import model_ref as R
from pass_scenes import host, lib, stream  # noqa: F401 (lib is a fixture)
from test_model_ops_cpu import STATS_V, stats_cases, texture_case
from util import assert_bit_equal, numpy_dot3_is_double_accumulated

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def c3(values, ctype=C.c_float):
    return (ctype * len(values))(*[float(v) for v in values])


def ok(rc, what):
    from cython3dmodelrenderer_amd import _capi
    _capi.check(rc, what)


# ---- crender_guro_illumination, crender_py_guro ----------------------------------------------------------------------

def _strips(H):
    """(at H = 5 the strip (3, H - 2) is empty: refused, in test_guro_refuses_bad_strips_and_writes_nothing)"""
    return [(y0, y1) for y0, y1 in ((0, H), (0, 1), (H - 1, H), (3, H - 2)) if y0 < y1]


@pytest.mark.parametrize("H,W", [(5, 7), (33, 67)])
def test_guro_on_painted_planes_strips_and_lights(lib, H, W):
    normals, color = R.painted_normals(H, H, W), R.painted_colors(H, H, W)
    d_n = dev(normals)
    for light in R.LIGHTS:
        l3 = R.light_vector(light)
        for y0, y1 in _strips(H):
            want = R.guro(color.copy(), normals, l3, y0, y1)
            d_c = dev(color)
            ok(lib.crender_guro_illumination(d_c.data_ptr(), d_n.data_ptr(), c3(l3), H, W, y0, y1, stream()), "guro")
            got = host(d_c)
            what = f"{H}x{W} light {light} rows [{y0}, {y1})"
            R.assert_equal_bits_or_nan(got[y0:y1], want[y0:y1], what)
            assert_bit_equal(got[:y0], color[:y0], what + ": rows above keep their bits")
            assert_bit_equal(got[y1:], color[y1:], what + ": rows below keep their bits")
    assert_bit_equal(host(d_n), normals, "the normals are only read")


def test_guro_refuses_bad_strips_and_writes_nothing(lib):
    from cython3dmodelrenderer_amd import _capi
    H, W = 5, 7
    normals, color = R.painted_normals(H, H, W), R.painted_colors(H, H, W)
    d_n, d_c = dev(normals), dev(color)
    for y0, y1 in ((2, 2), (3, H - 2), (3, 2), (0, H + 1), (-1, 3), (H, H)):
        rc = lib.crender_guro_illumination(d_c.data_ptr(), d_n.data_ptr(), c3((0, 0, -1)), H, W, y0, y1, stream())
        assert rc == _capi.EINVAL, (y0, y1, rc)
    assert_bit_equal(host(d_c), color, "a refused call writes nothing")


def test_guro_second_trip_of_the_grid(lib):
    """1025 x 1024 pixels: one row more than 4 096 blocks of 256 threads take in one trip."""
    H, W = 1025, 1024
    rng = np.random.default_rng(6)
    normals = rng.standard_normal((H, W, 3)).astype(f32)
    normals[::7, ::5] = R.painted_normals(2, 147, 205)
    color = rng.uniform(-300, 300, (H, W, 3)).astype(f32)
    l3 = R.light_vector(R.LIGHTS[3])
    d_n = dev(normals)
    for y0, y1 in ((0, H), (3, H - 2)):
        want = R.guro(color.copy(), normals, l3, y0, y1)
        assert (want[-3:] != color[-3:]).any()
        d_c = dev(color)
        ok(lib.crender_guro_illumination(d_c.data_ptr(), d_n.data_ptr(), c3(l3), H, W, y0, y1, stream()), "guro")
        R.assert_equal_bits_or_nan(host(d_c), want, f"rows [{y0}, {y1})")


@pytest.mark.parametrize("H,W", [(5, 7), (33, 67)])
def test_py_guro_on_painted_planes(lib, H, W):
    from cython3dmodelrenderer_amd.py.illumination import GuroIllumination
    normals = R.painted_normals(H, H, W)
    color = np.random.default_rng(H).integers(0, 256, (H, W, 3)).astype(np.uint8)
    color.reshape(-1)[:4] = [0, 255, 1, 254]
    d_n = dev(normals)
    for light in R.LIGHTS:
        with np.errstate(all="ignore"):
            g = GuroIllumination(light)
            want = color.copy()
            g.draw_illumination(want, normals)
        d_c = dev(color)
        g.draw_illumination_device(d_c, d_n)
        assert_bit_equal(host(d_c), want, f"{H}x{W} light {light}")


# ---- crender_present_u8 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (2, 9)])
def test_present_u8_on_the_value_table(lib, H, W):
    import torch
    vals, per = R.PRESENT_VALUES, H * W * 3
    for start in range(0, len(vals), per):                     # as many planes as hold the whole table
        plane = np.resize(np.roll(vals, -start), (H, W, 3)).astype(f32)
        d_p = dev(plane)
        for flip in (0, 1):
            out = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda:0")
            ok(lib.crender_present_u8(d_p.data_ptr(), out.data_ptr(), H, W, flip, stream()), "present")
            assert_bit_equal(host(out), R.present_u8(plane, flip), f"{H}x{W} from value {start}, flip_rows={flip}")
        assert_bit_equal(host(d_p), plane, "the plane is only read")


# ---- crender_model_shift, crender_model_scale, crender_model_scale3 --------------------------------------------------

# The first of each: as large as the vertices or larger, so that rounding the argument to float32 (2^-25 of it) is a
# fair part of an ulp of the result and the float32 and the float64 route differ on a fifth of the elements (after
# keep_position's `+ mean` too, which hides the difference for a small coefficient); asserted on the model below.
SHIFTS = ((1000.1, -777.7, 123.456), (0.1, 1e-9, 3e8), (-0.0, np.nan, np.inf))
COEFS = ((1000.37, -123.457, 77.7), (0.37, 1e-30, -1.0), (0.0, np.inf, np.nan), (0.37, 0.37, 0.37))
MODEL_V = (0, 1, 85, 86, 349_526)                               # 3 V = 2^20 + 2 at the last


def _share_differing(a, b):
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


@pytest.mark.parametrize("V", MODEL_V)
def test_model_shift(lib, V):
    v = R.special_vertices(np.random.default_rng(V), V)
    for s3 in SHIFTS:
        for is_f32 in (1, 0):
            want = R.shift(v, s3, not is_f32)
            d_v = dev(v)
            ok(lib.crender_model_shift(d_v.data_ptr(), V, c3(s3, C.c_double), is_f32, stream()), "shift")
            R.assert_equal_bits_or_nan(host(d_v), want, f"V={V} shift {s3} shift_is_float32={is_f32}")
        if V >= 85 and s3 == SHIFTS[0]:
            # the two modes are different arithmetic: the test cannot pass with the flag ignored
            assert _share_differing(R.shift(v, s3, True), R.shift(v, s3, False)) >= 0.01


@pytest.mark.parametrize("V", MODEL_V)
def test_model_scale_both_entries(lib, V):
    v = R.special_vertices(np.random.default_rng(V + 1), V)
    mean = np.array([9.5, -4.25, 2.0625], f32)
    d_mean = dev(mean)
    for co in COEFS:
        for keep in (1, 0):
            for is_f32 in (1, 0):
                want = R.scale(v, mean, co, not is_f32, keep)
                d_v = dev(v)
                ok(lib.crender_model_scale3(d_v.data_ptr(), V, d_mean.data_ptr(), c3(co, C.c_double), is_f32, keep,
                                            stream()), "scale3")
                R.assert_equal_bits_or_nan(host(d_v), want, f"V={V} scale3 {co} keep={keep} coef_is_float32={is_f32}")
            if V >= 85 and co == COEFS[0]:
                assert _share_differing(R.scale(v, mean, co, True, keep), R.scale(v, mean, co, False, keep)) >= 0.01
            for coef in dict.fromkeys(co):                      # the one-coefficient entry: float32 only
                d_v = dev(v)
                ok(lib.crender_model_scale(d_v.data_ptr(), V, d_mean.data_ptr(), C.c_float(coef), keep, stream()), "scale")
                R.assert_equal_bits_or_nan(host(d_v), R.scale(v, mean, (coef,) * 3, False, keep),
                                           f"V={V} scale {coef} keep={keep}")
    assert_bit_equal(host(d_mean), mean, "the mean is only read")


# ---- crender_model_stats ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", STATS_V)
def test_model_stats(lib, V):
    import torch
    for name, v in stats_cases(V):
        mean = R.mean_vertex(v)
        span = R.max_span(v, mean)
        d_v = dev(v)
        stats = torch.full((4,), 77.0, dtype=torch.float32, device="cuda:0")
        ok(lib.crender_model_stats(d_v.data_ptr(), V, stats.data_ptr(), stats.data_ptr() + 12, stream()), "stats")
        got = host(stats)
        R.assert_equal_bits_or_nan(got[:3], mean, f"V={V}, {name}: mean")
        R.assert_equal_bits_or_nan(got[3:], np.array([span], f32), f"V={V}, {name}: span")


# ---- crender_model_rotate --------------------------------------------------------------------------------------------

def _rotation(angles):
    from cython3dmodelrenderer_amd.data_structures.model import _rot2
    ax, ay, az = angles
    rx, ry, rz = np.eye(3), np.eye(3), np.eye(3)
    rx[1:, 1:] = _rot2(ax)
    ry[::2, ::2] = _rot2(ay)
    rz[:2, :2] = _rot2(az)
    return np.matmul(np.matmul(rx, ry), rz)


@pytest.mark.parametrize("V", [0, 1, 257, 1_048_640])
def test_model_rotate(lib, V):
    v = R.special_vertices(np.random.default_rng(V + 2), V)
    v[::3, 1] = v[::3, 0]                                       # x = y: the first two terms of `cancels` cancel exactly
    with_nan, huge, cancels = _rotation([33.3, 0.5, -271.0]), _rotation([10, -80, 0]), _rotation([10, -80, 0])
    with_nan[1, 2] = np.nan
    huge[0, 1] = 1e300
    cancels[0] = [1e300, -1e300, 1.0]
    for name, rot in (("identity", np.eye(3)), ("[-90, 180, 0]", _rotation([-90, 180, 0])),
                      ("[10, -80, 0]", _rotation([10, -80, 0])), ("a NaN", with_nan), ("1e300", huge),
                      ("1e300 and -1e300", cancels)):
        want = R.rotate(v, rot)
        d_v = dev(v)
        ok(lib.crender_model_rotate(d_v.data_ptr(), V, c3(rot.reshape(9), C.c_double), stream()), "rotate")
        R.assert_equal_bits_or_nan(host(d_v), want, f"V={V}, {name}")
    if V:
        # (x*1e300 - x*1e300) + z = z, but x*1e300 + (-x*1e300 + z) = 0: the grouping of the sum is part of what is
        # compared (between two rotations it shows only within 1e-16 of a float32 rounding boundary)
        x, y, z = (v[:, k].astype(f64) for k in range(3))
        with np.errstate(all="ignore"):
            right = (x * 1e300 + (y * -1e300 + z)).astype(f32)
        assert _share_differing(right, want[:, 0].copy()) >= 0.3


# ---- crender_model_vertex_normals ------------------------------------------------------------------------------------

def _vertex_normals(lib, v, f):
    """-> (normals, face normals, taken) of the C entry on a hand-built CSR."""
    import torch
    V, T = len(v), len(f)
    offs, occ = R.vertex_face_csr(f, V)
    assert offs.shape == (V + 1,) and occ.shape == (3 * T,) and offs[-1] == 3 * T
    assert T == 0 or (0 <= f.min() and f.max() < V and 0 <= occ.min() and occ.max() < T)
    d_v, d_f, d_offs, d_occ = dev(v), dev(f.astype(np.int32)), dev(offs), dev(occ)
    fn = torch.full((T, 3), 77.0, dtype=torch.float32, device="cuda:0")
    taken = torch.full((3 * T,), 77, dtype=torch.uint8, device="cuda:0")
    out = torch.full((V, 3), 77.0, dtype=torch.float32, device="cuda:0")
    ok(lib.crender_model_vertex_normals(d_v.data_ptr(), V, d_f.data_ptr(), T, d_offs.data_ptr(), d_occ.data_ptr(),
                                        fn.data_ptr(), taken.data_ptr(), out.data_ptr(), stream()), "vertex normals")
    assert_bit_equal(host(d_v), v, "the vertices are only read")
    return host(out), host(fn), host(taken)


def test_vertex_normals_on_the_edge_meshes(lib):
    from cython3dmodelrenderer_amd.data_structures.model import _vertex_normals as host_vertex_normals
    blas = numpy_dot3_is_double_accumulated()
    for name, v, f in R.edge_meshes():
        n, fn, taken = R.plain_f32_vertex_normals(v, f, full=True)
        got_n, got_fn, got_taken = _vertex_normals(lib, v, f)
        R.assert_equal_bits_or_nan(got_fn, fn, f"{name}: face normals")
        assert_bit_equal(got_taken, taken, f"{name}: taken")
        R.assert_equal_bits_or_nan(got_n, n, f"{name}: normals")
        if blas and len(v):
            with np.errstate(all="ignore"):
                R.assert_equal_bits_or_nan(got_n, host_vertex_normals(v, f), f"{name}: against the host Model")


def test_vertex_normals_second_trip_of_both_grids(lib):
    """1 048 640 disjoint triangles over 3 T vertices: the face and the vertex kernel both loop twice."""
    T = 1_048_640
    rng = np.random.default_rng(12)
    v = rng.standard_normal((3 * T, 3)).astype(f32)
    v[:9] = np.round(v[:9])
    v[9:12] = [[np.nan, 0, 0], [1, 2, 3], [3, 2, 1]]
    v[12:15] = 7.0
    f = rng.permutation(3 * T).reshape(T, 3).astype(np.int32)
    n, fn = R.vertex_normals_one_face_each(v, f)
    got_n, got_fn, got_taken = _vertex_normals(lib, v, f)
    R.assert_equal_bits_or_nan(got_fn, fn, "face normals")
    assert (got_taken == 1).all()
    R.assert_equal_bits_or_nan(got_n, n, "normals")


# ---- crender_model_gather, crender_model_texture_colors --------------------------------------------------------------

@pytest.mark.parametrize("T,n", [(0, 0), (0, 1), (1, 1), (1, 349_526), (349_526, 1), (349_526, 349_526)])
def test_model_gather(lib, T, n):
    import torch
    rng = np.random.default_rng(T + n)
    attr = R.special_vertices(rng, n)
    index = rng.integers(0, max(n, 1), (T, 3)).astype(np.int32)
    if T:
        index[0, 0], index[-1, -1] = n - 1, 0                   # the last and the first row
        assert 0 <= index.min() and index.max() < n
    d_attr, d_index = dev(attr), dev(index)
    out = torch.full((T, 3, 3), 77.0, dtype=torch.float32, device="cuda:0")
    ok(lib.crender_model_gather(d_attr.data_ptr(), d_index.data_ptr(), out.data_ptr(), T, stream()), "gather")
    R.assert_equal_bits_or_nan(host(out), R.gather(attr, index), f"T={T}, n={n}")


@pytest.mark.parametrize("n", [0, 1, 1_048_676])
@pytest.mark.parametrize("cols", [2, 3])
def test_model_texture_colors(lib, n, cols):
    import torch
    uv, tex = texture_case(n, cols)
    d_uv, d_tex = dev(uv), dev(tex)
    out = torch.full((n, 3), 77.0, dtype=torch.float32, device="cuda:0")
    ok(lib.crender_model_texture_colors(d_uv.data_ptr(), cols, n, d_tex.data_ptr(), tex.shape[0], tex.shape[1],
                                        out.data_ptr(), stream()), "texture colours")
    want = R.texture_colors(uv, tex)
    assert_bit_equal(host(out), want, f"n={n}, {cols} columns")
    if n > 1:
        assert len(np.unique(want.view([("", f32)] * 3))) == 15           # every texel of the 3 x 5 texture


# ---- crender_tile_order_keys -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [0, 1, 257, 1_048_640])
def test_tile_order_keys(lib, oracle, T):
    import torch
    from cython3dmodelrenderer_amd import _capi
    for w, h in ((4, 4), (300, 200), (1024, 1024), (8192, 8192)):
        tri = R.key_triangles(np.random.default_rng(T + w), T, max(w, h))
        P = oracle.projection_matrix(45.0, 0.1, 1000.0, h, w)
        d_tri = dev(tri)
        keys = torch.full((T,), 0x77777777, dtype=torch.int32, device="cuda:0")
        ok(lib.crender_tile_order_keys(d_tri.data_ptr(), T, _capi.f32_16(P), w, h, keys.data_ptr(), stream()), "keys")
        got = host(keys).view(np.uint32)
        assert_bit_equal(got.view(np.int32), R.tile_order_keys(tri, P, w, h).view(np.int32), f"T={T}, {w} x {h}")
        if w == 4:
            assert not got.any()
        # the prefix property the order relies on: key >> 2k is the key of the cell 2^k times coarser
        x, y = R.tile_order_cells(tri, P, w, h)
        for k in range(1, 5):
            assert (got >> np.uint32(2 * k) == R.morton15(x >> (2 + k), y >> (2 + k))).all(), (T, w, h, k)


# ---- sessions: DeviceModel against the host Model --------------------------------------------------------------------

def _same_bits(got, want):
    got, want = np.atleast_1d(np.asarray(got, f32)), np.atleast_1d(np.asarray(want, f32))
    return int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())


def run_session(seed, device_model_class, report):
    """20 drawn steps on V = 500, T = 900; after each, `report(step, what, differing, of)` for the vertices, the
    vertices by triangles, the mean, the span and the normals by triangles."""
    from cython3dmodelrenderer_amd.data_structures.model import Model, _vertex_normals as host_vertex_normals
    rng = np.random.default_rng(1000 + seed)
    V, T = 500, 900
    vertices = (rng.standard_normal((V, 3)) * [3.0, 1.0, 0.5] + [10.0, -4.0, 2.0]).astype(f32)
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    blas = numpy_dot3_is_double_accumulated()
    hostm, devm = Model(vertices, faces), device_model_class(Model(vertices, faces))
    for step in range(20):
        op = ("shift", "scale keep", "scale", "rotate", "rotate on host", "mean", "span")[rng.integers(0, 7)]
        kinds = R.argument_kinds(rng.uniform(0.5, 1.5, 3) * rng.choice([-1, 1], 3), rng.integers(1, 3, 3))
        name, arg = kinds[rng.integers(0, len(kinds))]
        what = f"seed {seed} step {step}: {op}"
        if op == "shift":
            what += f" by a {name}"
            hostm.shift(arg)
            devm.shift(arg)
        elif op.startswith("scale"):
            what += f" by a {name}"
            hostm.scale(arg, keep_position=op == "scale keep")
            devm.scale(arg, keep_position=op == "scale keep")
        elif op == "rotate on host":
            angles = [float(a) for a in rng.uniform(-180, 180, 3)]
            hostm.rotate(angles)
            devm.rotate(angles, on_host=True)
        elif op == "rotate":
            angles = [float(a) for a in rng.uniform(-180, 180, 3)]
            before = host(devm._vertices)
            hostm.rotate(angles)
            devm.rotate(angles)
            dv, dn = host(devm._vertices), host(devm._normals)
            R.assert_equal_bits_or_nan(dv, R.rotate(before, _rotation(angles)), what + ": the spelled float64 sums")
            R.assert_equal_bits_or_nan(dn, R.plain_f32_vertex_normals(dv, faces), what + ": the spelled normals")
            # numpy's matmul belongs to its BLAS: as in test_device_model_rotate_and_normals, at most 2 vertices
            assert (dv.view(np.uint32) != hostm._vertices.view(np.uint32)).any(axis=1).sum() <= 2, what
            if blas:
                report(step, what + ": normals of the device's vertices", _same_bits(dn, host_vertex_normals(dv, faces)),
                       dn.size)
            hostm._set_geometry(dv.copy(), hostm._triangles_vertices, dn.copy(), hostm._triangles_vertices, recalc=False)
        report(step, what + ": vertices", _same_bits(host(devm._vertices), hostm._vertices), 3 * V)
        report(step, what + ": vertices by triangles",
               _same_bits(host(devm._vertices_by_triangles), hostm._vertices_by_triangles), 9 * T)
        report(step, what + ": normals by triangles",
               _same_bits(host(devm._normals_by_triangles), hostm._normals_by_triangles), 9 * T)
        if op in ("mean", "span") or step % 5 == 4:
            report(step, what + ": mean", _same_bits(devm.get_mean_vertex(), hostm.get_mean_vertex()), 3)
            report(step, what + ": span", _same_bits(devm.get_max_span(), hostm.get_max_span()), 1)


@pytest.mark.parametrize("seed", range(8))
def test_device_model_sessions(lib, seed):
    from cython3dmodelrenderer_amd.data_structures import DeviceModel

    def report(step, what, differing, of):
        assert differing == 0, f"{what}: {differing} of {of} elements differ"
    run_session(seed, DeviceModel, report)
