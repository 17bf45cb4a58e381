"""The numpy models of tests/model_ref.py pinned against what they restate, with no GPU: GuroIllumination and the
oracle's restatement of it, numpy's ``astype('uint8')``, the host ``Model``'s shift, scale, mean, span and vertex
normals — at the operand edges the GPU file (tests/test_model_ops_gpu.py) then holds the kernels to — and
``host_arithmetic_is_float64``, the rule by which ``DeviceModel`` follows numpy's promotion."""
import time

import numpy as np
import pytest

import model_ref as R
from util import assert_bit_equal, numpy_dot3_is_double_accumulated

f32 = np.float32
STATS_V = (1, 2, 32, 33, 34, 64, 65, 66, 1000, 262_401)


def _model(vertices, faces=None):
    from cython3dmodelrenderer_amd.data_structures.model import Model
    faces = np.zeros((1, 3), np.int32) if faces is None else faces
    with np.errstate(all="ignore"):
        return Model(vertices, faces, normals=np.zeros((1, 3), f32), triangles_normals=np.zeros((1, 3), np.int32),
                     recalculate_normals=False)


# ---- Guro ------------------------------------------------------------------------------------------------------------

def test_guro_model_is_numpys_and_the_oracles(oracle):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    rng = np.random.default_rng(3)
    S = R.SPECIALS
    every = np.stack(np.meshgrid(S, S, S, indexing="ij"), -1).reshape(-1, 3)           # every triple: 8 000
    drawn = S[rng.integers(0, len(S), (12_000, 3))]
    gauss = rng.standard_normal((4_000, 3)).astype(f32)
    normals = np.concatenate([every, drawn, gauss]).reshape(-1, 1, 3)
    color = rng.uniform(-300, 300, normals.shape).astype(f32)
    color[:8, 0] = [[-7.5, 0.0, -0.0], [np.inf, 255.0, 1.0]] * 4
    color[8:8008:7, 0, 1] = np.inf
    for light in R.LIGHTS:
        want = color.copy()
        with np.errstate(all="ignore"):
            GuroIllumination(light).draw_illumination(want, normals)
        l3 = R.light_vector(light)
        with np.errstate(all="ignore"):
            assert_bit_equal(l3, oracle.guro_light(light), "the light vector")
        got = R.guro(color.copy(), normals, l3)
        assert np.isnan(want).any() and (want == 0).any() and np.isinf(want).any()
        R.assert_equal_bits_or_nan(got, want, f"light {light}: the model against numpy")
        with np.errstate(all="ignore"):
            R.assert_equal_bits_or_nan(oracle.guro(color.copy(), normals, light), got, f"light {light}: against the oracle")
    # a strip leaves the rows outside it alone
    plane_n, plane_c = R.painted_normals(1, 5, 7), R.painted_colors(1, 5, 7)
    got = R.guro(plane_c.copy(), plane_n, R.light_vector(R.LIGHTS[3]), 1, 3)
    whole = R.guro(plane_c.copy(), plane_n, R.light_vector(R.LIGHTS[3]))
    assert_bit_equal(got[:1], plane_c[:1], "rows above the strip")
    assert_bit_equal(got[3:], plane_c[3:], "rows below the strip")
    R.assert_equal_bits_or_nan(got[1:3], whole[1:3], "the strip")


def test_painted_planes_hold_what_the_gpu_tests_need():
    for H, W in ((5, 7), (33, 67)):
        n, c = R.painted_normals(H, H, W), R.painted_colors(H, H, W)
        flat = n.reshape(-1)
        for s in R.SPECIALS:
            assert ((flat == s) & (np.signbit(flat) == np.signbit(s))).any() or (np.isnan(s) and np.isnan(flat).any())
        cf = c.reshape(-1)
        assert cf[0] == -7.5 and cf[1] == 0 and not np.signbit(cf[1]) and np.signbit(cf[2]) and np.isinf(cf[3])


# ---- presentation ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [17, 1024])
def test_present_model_is_numpys_cast(n):
    """(numpy may take another loop for the longer array: both are the x86-64 truncating cast on numpy 2.2.6)"""
    assert len(R.PRESENT_VALUES) == 17
    vals = np.resize(R.PRESENT_VALUES, n).astype(f32)
    with np.errstate(invalid="ignore"):
        want = vals.astype("uint8")
    assert (R.present_u8(vals, False) == want).all(), (vals[R.present_u8(vals, False) != want])
    plane = np.resize(R.PRESENT_VALUES, (3, 5, 3)).astype(f32)
    with np.errstate(invalid="ignore"):
        assert (R.present_u8(plane, True) == plane[::-1].astype("uint8")).all()


# ---- promotion, shift and scale --------------------------------------------------------------------------------------

def _kinds():
    return R.argument_kinds((0.1, 0.37, -1.25))


def test_promotion_rule_is_numpys():
    from cython3dmodelrenderer_amd.data_structures.device_model import host_arithmetic_is_float64
    v = np.ones((4, 3), f32)
    seen = set()
    for name, arg in _kinds():
        want = (v + arg).dtype
        assert want in (np.float32, np.float64), name
        assert host_arithmetic_is_float64(arg) == (want == np.float64), name
        inplace = v.copy()
        inplace *= arg                                           # Model.scale multiplies in place: same rule
        assert inplace.dtype == np.float32
        seen.add(want == np.float64)
    assert seen == {False, True}
    for refused in (1j, np.complex64(1), "abc", None, [None, 1, 2], np.longdouble(1), {"a": 1}):
        with pytest.raises(TypeError):
            host_arithmetic_is_float64(refused)


def test_shift_and_scale_models_are_the_host_models():
    from cython3dmodelrenderer_amd.data_structures.device_model import host_arithmetic_is_float64
    rng = np.random.default_rng(17)
    vertices = rng.standard_normal((1000, 3)).astype(f32)
    differ = {}
    for name, arg in _kinds():
        in_double = host_arithmetic_is_float64(arg)
        a3 = np.broadcast_to(np.asarray(arg).astype(np.float64 if in_double else f32), (3,)).astype(np.float64)
        m = _model(vertices.copy())
        m.shift(arg)
        assert_bit_equal(m._vertices, R.shift(vertices, a3, in_double), f"shift by a {name}")
        raw = np.broadcast_to(np.asarray(arg, np.float64), (3,))           # the other route, from the argument as it came
        differ[name, "shift"] = int((R.shift(vertices, raw, not in_double).view(np.uint32) !=
                                     m._vertices.view(np.uint32)).sum())
        for keep in (True, False):
            m = _model(vertices.copy())
            mean = m.get_mean_vertex().copy()
            m.scale(arg, keep_position=keep)
            assert_bit_equal(m._vertices, R.scale(vertices, mean, a3, in_double, keep), f"scale by a {name}, keep={keep}")
        differ[name, "scale"] = int((R.scale(vertices, mean, raw, not in_double, False).view(np.uint32) !=
                                     m._vertices.view(np.uint32)).sum())
    # the two routes are different arithmetic where the argument is no float32: a rule that took the other one fails
    assert differ["Python float", "shift"] >= 30 and differ["np.float64 scalar", "scale"] >= 30, differ
    assert differ["float32 array", "shift"] <= 3 and differ["float32 array", "scale"] == 0, differ


# ---- mean vertex and max span ----------------------------------------------------------------------------------------

def stats_cases(V):
    """-> [(name, vertices)]: what crender_model_stats is held to at V vertices."""
    rng = np.random.default_rng(V)
    base = (rng.standard_normal((V, 3)) * [3.0, 1.0, 0.5] + [1000.0, -4000.0, 250.0]).astype(f32)
    out = [("Gaussian on a large offset", base), ("all -0", np.full((V, 3), -0.0, f32))]
    for row in sorted({0, V - 1, 17, 40}):
        if row < V:
            v = base.copy()
            v[row, row % 3] = np.nan
            out.append((f"a NaN at row {row}", v))
    v = base.copy()
    v[V // 2, 1] = np.inf
    out.append(("an inf", v))
    return out


@pytest.mark.parametrize("V", STATS_V)
def test_stats_models_are_the_host_models(V):
    for name, v in stats_cases(V):
        m = _model(v.copy())
        mean = R.mean_vertex(v)
        R.assert_equal_bits_or_nan(mean, m.get_mean_vertex(), f"V={V}, {name}: mean")
        R.assert_equal_bits_or_nan(np.array(R.max_span(v, mean)), np.array(f32(m.get_max_span())), f"V={V}, {name}: span")
        if "NaN" in name:
            assert np.isnan(mean).sum() == 1 and np.isnan(R.max_span(v, mean))
        if name == "an inf":
            assert np.isinf(mean[1]) and np.isnan(R.max_span(v, mean))
        if name == "all -0":
            assert not np.signbit(mean).any() and R.max_span(v, mean) == 0         # add.reduce starts from +0


# ---- vertex normals --------------------------------------------------------------------------------------------------

def test_normal_models_are_the_host_models_on_the_edge_meshes():
    from cython3dmodelrenderer_amd.data_structures.model import _vertex_normals
    blas = numpy_dot3_is_double_accumulated()
    for name, v, f in R.edge_meshes():
        n, fn, taken = R.plain_f32_vertex_normals(v, f, full=True)
        assert n.shape == v.shape and fn.shape == f.shape and taken.shape == (f.size,)
        if blas and len(v):
            with np.errstate(all="ignore"):
                R.assert_equal_bits_or_nan(n, _vertex_normals(v, f), name)
        if name.startswith("first"):
            assert not n[[0, 3, 6]].any() and n[[1, 2, 4, 5]].any(axis=1).all()
        if name == "a fan of 200 faces with distinct normals":
            assert taken[:200].all()
        if name == "a fan of 64 coplanar faces":
            assert taken[:64].sum() == 1
        if name == "corners at 1e20":
            assert np.isnan(n).any()
        if name == "triangles of side 1e-12":
            assert (fn != 0).any() and (np.abs(fn) < 1e-20).all()            # not normalised
    # every vertex in exactly one face: the vectorised model is the loop's
    rng = np.random.default_rng(2)
    T = 400
    v = rng.standard_normal((3 * T, 3)).astype(f32)
    v[:9] = np.round(v[:9])                                                   # axis-aligned: zeros of either sign
    v[9:12] = [[np.nan, 0, 0], [1, 2, 3], [3, 2, 1]]
    v[12:15] = 7.0                                                            # no area
    f = rng.permutation(3 * T).reshape(T, 3).astype(np.int32)
    f[:5] = np.arange(15).reshape(5, 3)
    rest = np.setdiff1d(np.arange(3 * T), np.arange(15))
    f[5:] = rng.permutation(rest).reshape(T - 5, 3)
    n, fn, taken = R.plain_f32_vertex_normals(v, f, full=True)
    n1, fn1 = R.vertex_normals_one_face_each(v, f)
    assert taken.all()
    R.assert_equal_bits_or_nan(n1, n, "vectorised against the loop: normals")
    R.assert_equal_bits_or_nan(fn1, fn, "vectorised against the loop: face normals")
    if blas:
        with np.errstate(all="ignore"):
            R.assert_equal_bits_or_nan(n1, _vertex_normals(v, f), "vectorised against the host Model")


def test_boundary_pairs_search():
    """Pairs of unit normals on which the two spellings of the dot decide differently: 60 of either kind (the cap)
    in a draw of 40 000 coplanar pairs here, which holds 1 128 and 1 943 of them, in 0.13 s."""
    t0 = time.perf_counter()
    v, f, kind = R.boundary_pairs()
    spent = time.perf_counter() - t0
    print(f"{(kind == 0).sum()} + {(kind == 1).sum()} boundary pairs in {spent:.2f} s")
    assert (kind == 0).sum() >= 20 and (kind == 1).sum() >= 20
    fn = R.face_normals(v, f)
    n1, n2 = fn[0::2], fn[1::2]
    p = (n1 * n2).astype(f32)
    plain = (p[:, 0] + p[:, 1]) + p[:, 2]
    dd = R._dot3_rows(n1, n2)
    assert ((dd >= 1) != (plain >= 1)).all() and ((dd >= 1) == (kind == 0)).all()
    # the shared corner's decision is the double-accumulated one
    _, _, taken = R.plain_f32_vertex_normals(v, f, full=True)
    offs, _ = R.vertex_face_csr(f, len(v))
    second = taken[offs[0:-1:5] + 1]                                          # the shared corners are vertices 0, 5, ...
    assert (second == (kind == 1)).all()


# ---- texture colours, Morton keys ------------------------------------------------------------------------------------

def test_texture_colour_model_is_the_host_models():
    from cython3dmodelrenderer_amd.data_structures.model import Model
    for cols in (2, 3):
        uv, tex = texture_case(2000, cols)
        with np.errstate(all="ignore"):
            m = Model(np.zeros((1, 3), f32), np.zeros((1, 3), np.int32), uv.tolist(), np.zeros((1, 3), np.int32), tex)
        assert_bit_equal(R.texture_colors(uv, tex), m._colors, f"{cols} columns")


def texture_case(n, cols, th=3, tw=5):
    """-> (uv float32 [n][cols], texture uint8 [th][tw][3]) with the special rows of the parity test."""
    rng = np.random.default_rng(n + cols)
    tex = rng.integers(0, 256, (th, tw, 3)).astype(np.uint8)
    uv = rng.uniform(-0.25, 1.25, (n, cols)).astype(f32)
    if n >= 70:
        uv[:40, :2] = rng.integers(0, 2, (40, 2))
        uv[40:60, :2] = f32(1.0) - f32(2.0) ** -rng.integers(1, 25, (20, 2))
        uv[60:70, :2] = [[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [0.5, -np.inf], [3e9, 0.5], [0.5, -3e9],
                         [1e38, 1e38], [-1e38, -1e38], [2.0 ** 31 / tw, 0.5], [0.5, 1 - 2.0 ** 31 / th]]
        uv[n - 1, :2] = [0.999, 0.001]
    return uv, tex


def test_projection_model_is_the_oracles_and_the_keys_interleave(oracle):
    rng = np.random.default_rng(9)
    for w, h in ((4, 4), (300, 200), (1024, 1024), (8192, 8192)):
        P = oracle.projection_matrix(45.0, 0.1, 1000.0, h, w)
        tri = R.key_triangles(rng, 400, max(w, h))
        R.assert_equal_bits_or_nan(R.project_rows(tri.reshape(-1, 3), P, w, h).reshape(-1, 3, 3),
                                   oracle.project(tri, P, w, h), f"{w} x {h}: projection")
        x, y = R.tile_order_cells(tri, P, w, h)
        assert x.min() == 0 and x.max() == w - 1 and y.min() == 0 and y.max() == h - 1       # off all four sides
        keys = R.tile_order_keys(tri, P, w, h)
        if w == 4:
            assert not keys.any()
        else:
            assert len(np.unique(keys)) > 50
        for k in range(5):
            assert (keys >> np.uint32(2 * k) == R.morton15(x >> (2 + k), y >> (2 + k))).all()
    assert R.morton15([0b101, 0, 0x7FFF, 0xFFFF], [0, 0b11, 0, 0]).tolist() == [0b010001, 0b1010, 0x15555555, 0x15555555]
    assert R.morton15([0], [0x7FFF]).tolist() == [0x2AAAAAAA]
