"""The contour edges without a GPU: the header against the binding and the library, the entry point's argument checks,
``wireframe.edge_partners`` on a hand-built mesh and against ``feature_edges``, the host model the GPU tests compare
with (tests/contour_ref.py) pinned by counts on T-Rex and by identities on generated meshes, and the argument checks of
``contour_edges`` and ``Renderer(wireframe={"contours": True, ...})``."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import contour_ref
import outline_ref
from pass_scenes import Frame, capi, recording_filler, trex_fixture  # noqa: F401 (fixtures)
from util import LIBRARY_SOURCES, UNIT_KEYS, other_symbols, sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTOUR_ARGTYPES = [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                    C.c_int, C.c_int, C.c_uint, C.c_void_p]
FILL = (30.0, 35.0, 40.0)


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_contours_symbol_is_declared_exported_and_bound(capi):
    from cython3dmodelrenderer_amd import _build
    header = open(os.path.join(ROOT, "include", "crender_wire.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert "crender_wire_contours" in declared and declared == set(capi.UNIT_SIGNATURES["wire"])
    assert not declared & other_symbols(capi, "wire")
    res, args = capi.UNIT_SIGNATURES["wire"]["crender_wire_contours"]
    assert res == C.c_int and args == CONTOUR_ARGTYPES
    assert capi.load().crender_wire_contours.argtypes == CONTOUR_ARGTYPES
    decl = re.search(r"CRENDER_API int crender_wire_contours\((.*?)\);", header, re.S).group(1)
    params = [" ".join(a.split()) for a in decl.split(",")]
    assert len(params) == len(args) == 12
    assert params == ["const float *d_tri", "int64_t T", "const uint32_t *d_pos_of", "const float *P16", "const int32_t *d_partners",
                      "const uint8_t *d_static", "int8_t *d_facing", "uint8_t *d_edges", "int H", "int W", "unsigned flags",
                      "void *stream"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert "crender_wire_contours" in set(re.findall(r" T (crender_\w+)", out))
    flag = re.search(r"#define CRENDER_WIRE_CONTOUR_BORDERS (\d+)u", header)
    assert int(flag.group(1)) == capi.WIRE_CONTOUR_BORDERS == contour_ref.BORDERS == 1
    # the feature lives in the wire unit as it was: no new unit, no new source, no new ABI, the same fingerprint
    assert capi.ABI_VERSION == 6
    assert _build.source_sha16() == "35a9bf480abfca1e"
    assert _build.library_sources() == LIBRARY_SOURCES
    assert list(_build.UNITS) == UNIT_KEYS
    assert _build.UNITS["wire"][0] == ["wireframe.hip"]
    unit = open(os.path.join(_build.SRC_DIR, "wireframe.hip")).read()
    assert "k_wire_facing" in unit and "k_wire_contour_mask" in unit
    # the projection is the rasterizer's, called: the kernel restates neither it nor the gather
    body = unit[unit.index("void k_wire_facing"):unit.index("void k_wire_contour_mask")]
    # (both through winner_pass.h's winner_triangle, once per triangle)
    assert body.count("winner_triangle(tri, q, P)") == 1 and "asm" not in body
    assert "project_vertex(" not in unit and "gather_corners(" not in unit


def test_contours_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first, or has T = 0

    def contours(tri=fake, T=4, pos_of=None, P=P, partners=fake, static=None, facing=fake, edges=fake, H=8, W=8, flags=0):
        return L.crender_wire_contours(tri, T, pos_of, P, partners, static, facing, edges, H, W, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(P=None), dict(partners=None), dict(facing=None), dict(edges=None)):
        assert contours(**kw) == E and "is NULL" in text(), kw
    assert contours(tri=None) == E and "NULL with T > 0" in text()
    for bad in (-1, -2 ** 40):
        assert contours(T=bad) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert contours(**kw) == E and "H or W is below 1" in text(), kw
    for flags in (2, 3, 4, 0x80000000):
        assert contours(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_wire_contours")
    # without triangles there is nothing to launch
    assert contours(T=0, tri=None) == capi.OK
    assert contours(T=0, tri=None, static=fake, pos_of=fake, flags=1, H=1, W=1) == capi.OK
    assert contours(T=0, flags=2) == E


# ---- the partner table -----------------------------------------------------------------------------------------

def _check_round_trip(partners):
    """Every entry that names a partner is named back by it, with the same s."""
    T = len(partners)
    t, e = np.nonzero(partners >= 0)
    v = partners[t, e]
    p, s = v >> 1, v & 1
    assert (p < T).all()
    back = partners[p]                                  # [N, 3]
    assert (((back >> 1) == t[:, None]) & ((back & 1) == s[:, None]) & (back >= 0)).any(1).all()


def test_edge_partners_on_a_hand_built_mesh():
    import torch
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    tri, want = contour_ref.hand_mesh()
    got = edge_partners(tri)
    assert got.dtype == np.int32 and got.shape == (8, 3)
    assert got.tolist() == want.tolist()
    _check_round_trip(got)
    # the torch form (here on the host's tensors) gives the same table, on the tensor's device
    dev = edge_partners(torch.from_numpy(tri))
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.int32 and dev.device == torch.device("cpu")
    assert dev.numpy().tolist() == want.tolist()
    # an entry below 0 is what feature_edges(tri, 180) marks as a border or an edge of several faces.  (That function
    # also marks the edges of a face without area, whatever their partners: triangle 5 here, which is compared apart.)
    marked = ((feature_edges(tri, 180.0)[:, None] >> np.arange(3)) & 1).astype(bool)
    assert (marked[got < 0]).all()
    flat = np.zeros(8, bool)
    flat[5] = True
    assert ((got < 0) == marked)[~flat].all()
    assert marked[5].all() and (got[5] < 0).tolist() == [True, False, False]
    # order, shape and size
    perm = np.random.default_rng(3).permutation(8)
    moved = edge_partners(tri[perm])
    inv = np.argsort(perm)
    assert ((moved < 0) == (got[perm] < 0)).all() and (moved[moved < 0] == got[perm][moved < 0]).all()
    at = moved >= 0
    assert (perm[moved[at] >> 1] == (got[perm][at] >> 1)).all() and ((moved[at] & 1) == (got[perm][at] & 1)).all()
    assert inv[perm].tolist() == list(range(8))
    assert edge_partners(tri[:0]).shape == (0, 3) and edge_partners(tri[:0]).dtype == np.int32
    assert tuple(edge_partners(torch.from_numpy(tri[:0])).shape) == (0, 3)
    for bad in (np.zeros((4, 3), np.float32), np.zeros((4, 3, 2), np.float32)):
        with pytest.raises(ValueError, match=r"\[T, 3, 3\]"):
            edge_partners(bad)
    with pytest.raises(ValueError, match=r"float32 \[T, 3, 3\]"):
        edge_partners(torch.zeros((4, 3, 3), dtype=torch.float64))


def test_edge_partners_and_feature_edges_on_trex(trex):
    import torch
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    got = edge_partners(trex.tri)
    # closed and consistently wound: every half-edge has one partner, running the other way
    assert got.shape == (13814, 3) and (got >= 0).all() and not (got & 1).any()
    _check_round_trip(got)
    assert len({tuple(sorted((t, int(v) >> 1))) for t, row in enumerate(got) for v in row}) == 20721
    assert not feature_edges(trex.tri, 180.0).any()
    assert np.array_equal(edge_partners(torch.from_numpy(trex.tri)).numpy(), got)
    # feature_edges shares the sort with the table and keeps its bits: the digests of its masks before it did
    for angle, digest in ((30.0, "06655f19f9be5333c9ecc7a65aa693c1708f1630e3324255b3907d1dc3d74bf3"),
                          (5.0, "2f878cd8a69cc4a7282dfc175721bf551a1d3449e188cb982a057d61bcb248df")):
        assert sha(feature_edges(trex.tri, angle)) == digest, angle
    assert int(np.unpackbits(feature_edges(trex.tri, 30.0)).sum()) == 10122          # of 41 442 half-edges


# ---- the model on T-Rex ----------------------------------------------------------------------------------------

trex = trex_fixture(Frame)


def _vertex_degrees(tri, bits):
    """How many drawn EDGES touch every vertex that a drawn edge touches."""
    deg = {}
    for a, b in contour_ref.edge_keys(tri, bits):
        deg[a] = deg.get(a, 0) + 1
        deg[b] = deg.get(b, 0) + 1
    return deg


def _check_symmetric(partners, on):
    """Both half-edges of every drawn edge that has a partner are drawn."""
    t, e = np.nonzero(on & (partners >= 0))
    p = partners[t, e] >> 1
    back = ((partners[p] >> 1) == t[:, None]) & (partners[p] >= 0)
    assert (back & on[p]).any(1).all()


def test_the_counts_on_trex(trex):
    """T-Rex at 256^2 in the fixture's pose, under the oracle's projection matrix."""
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    P = trex.cam.proj_mat
    partners = edge_partners(trex.tri)
    bits, face = contour_ref.contour_edges(trex.tri, P, 256, 256, partners)
    assert bits.dtype == np.uint8 and face.dtype == np.int8
    assert ((face == 1).sum(), (face == -1).sum(), (face == 0).sum()) == (7235, 6579, 0)
    on = contour_ref.contours(face, partners)
    assert int(on.sum()) == 4810 and len(contour_ref.edge_keys(trex.tri, bits)) == 2405
    assert not (bits >> 3).any()
    # no facing is 0 on a closed, consistently wound mesh: the contour is a set of closed loops
    _check_symmetric(partners, on)
    deg = _vertex_degrees(trex.tri, bits)
    assert deg and all(d % 2 == 0 for d in deg.values())
    # there are no borders to add, and a static mask is kept
    assert np.array_equal(contour_ref.contour_edges(trex.tri, P, 256, 256, partners, borders=True)[0], bits)
    static = feature_edges(trex.tri, 30.0)
    both = contour_ref.contour_edges(trex.tri, P, 256, 256, partners, static=static | np.uint8(0xF8), borders=True)[0]
    assert np.array_equal(both, bits | static) and not (both >> 3).any()
    held = len(contour_ref.edge_keys(trex.tri, bits & static))
    assert (held, len(contour_ref.edge_keys(trex.tri, static)), len(contour_ref.edge_keys(trex.tri, both))) == (1742, 5061, 5724)
    # what that draws under outline=True: line pixels on the background and on the body, without and with the contours
    want = {(1.0, False): (583, 4250), (1.0, True): (745, 4454), (3.0, False): (1264, 6739), (3.0, True): (1557, 6962)}
    for (width, contours), (background_on, covered_on) in want.items():
        c = {}
        outline_ref.wire_pass(trex.cam.color_buffer, trex.cam.winner, trex.cam.z_buffer, trex.tri, P, width=width, fill=FILL,
                              edges=both if contours else static, counts=c)
        assert (c["background_on"], c["covered_on"]) == (background_on, covered_on), (width, contours, c)


# ---- generated meshes ------------------------------------------------------------------------------------------

def _P(oracle, H, W):
    return oracle.OracleFiller(H, W, fov=45.0).proj_mat


def test_flipping_windings_keeps_the_contour_edges(oracle):
    from cython3dmodelrenderer_amd.wireframe import edge_partners
    H, W = 96, 160
    P = _P(oracle, H, W)
    rng = np.random.default_rng(11)
    for angles in ((0, 0, 0), (25, 40, 10), (-70, 15, 200)):
        tri = contour_ref.place(contour_ref.uv_sphere(), angles)
        assert len(tri) == 288
        partners = edge_partners(tri)
        assert (partners >= 0).all() and not (partners & 1).any()
        bits, face = contour_ref.contour_edges(tri, P, W, H, partners)
        assert not (face == 0).any() and (face == 1).any() and (face == -1).any()
        edges = contour_ref.edge_keys(tri, bits)
        assert len(edges) >= 16
        _check_symmetric(partners, contour_ref.contours(face, partners))
        assert all(d % 2 == 0 for d in _vertex_degrees(tri, bits).values())
        flip = rng.uniform(size=len(tri)) < 1 / 3
        assert 60 < flip.sum() < 130
        turned = tri.copy()
        turned[flip] = tri[flip][:, [0, 2, 1]]
        again = edge_partners(turned)
        assert (again >= 0).all() and (again & 1).any() and not (again & 1).all()
        _check_round_trip(again)
        bits2, face2 = contour_ref.contour_edges(turned, P, W, H, again)
        assert (face2[flip] == -face[flip]).all() and (face2[~flip] == face[~flip]).all()
        assert contour_ref.edge_keys(turned, bits2) == edges
        # under the table of the unturned mesh the turned one draws other edges: s is what keeps them
        assert contour_ref.edge_keys(turned, contour_ref.mask(face2, again & ~np.int32(1))) != edges


def test_an_open_cylinder_gets_its_rims_with_borders(oracle):
    from cython3dmodelrenderer_amd.wireframe import edge_partners
    H, W = 96, 160
    P = _P(oracle, H, W)
    tri = contour_ref.place(contour_ref.open_cylinder(), (20, 30, 10))
    partners = edge_partners(tri)
    assert len(tri) == 128 and (partners == -1).sum() == 32 and not (partners == -2).any()
    u = tri.view(np.uint32)
    rim = set()
    for t, e in zip(*np.nonzero(partners == -1)):
        a, b = tuple(u[t, e]), tuple(u[t, (e + 1) % 3])
        rim.add((min(a, b), max(a, b)))
    assert len(rim) == 32
    plain = contour_ref.edge_keys(tri, contour_ref.contour_edges(tri, P, W, H, partners)[0])
    rimmed = contour_ref.edge_keys(tri, contour_ref.contour_edges(tri, P, W, H, partners, borders=True)[0])
    assert plain and not plain & rim and rimmed == plain | rim


def test_a_junk_table_sets_nothing(oracle):
    H, W = 96, 160
    P = _P(oracle, H, W)
    tri = contour_ref.place(contour_ref.uv_sphere(), (25, 40, 10))
    T = len(tri)
    face = contour_ref.facing(tri, P, W, H)
    for junk in (-3, 2 * T, 2 * T + 1, 2 ** 31 - 1, -2 ** 31):
        table = np.full((T, 3), junk, np.int32)
        for flags in (0, contour_ref.BORDERS):
            assert not contour_ref.mask(face, table, None, flags).any(), (junk, flags)
    # facing 0 at either side never makes a contour, under either s
    pair = np.int32([[2, -1, -1], [0, -1, -1]])
    for f0, f1 in ((0, 1), (1, 0), (0, 0), (0, -1)):
        for s in (0, 1):
            assert not contour_ref.mask(np.int8([f0, f1]), pair | s).any()
    assert contour_ref.mask(np.int8([1, -1]), pair).tolist() == [1, 1] and not contour_ref.mask(np.int8([1, 1]), pair).any()
    assert contour_ref.mask(np.int8([1, 1]), pair | 1).tolist() == [1, 1] and not contour_ref.mask(np.int8([1, -1]), pair | 1).any()
    assert contour_ref.mask(np.int8([1, 1]), pair, None, contour_ref.BORDERS).tolist() == [6, 6]
    # a d_pos_of entry beyond T: the facing is 0
    pos_of = np.arange(T, dtype=np.uint32)
    pos_of[::5] = np.uint32([T, T + 3, 2 ** 32 - 1] * T)[:len(pos_of[::5])]
    moved = contour_ref.facing(tri, P, W, H, pos_of)
    assert not moved[::5].any() and (np.delete(moved, np.s_[::5]) == np.delete(face, np.s_[::5])).all()


# ---- the Python layer ------------------------------------------------------------------------------------------

def _stub(T=5, **kw):
    from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses
    stub = SimpleNamespace(_pipeline=None, winner_buffer=None, _inputs=(np.zeros((T, 3, 3), np.float32),), _last_flags=1,
                           device="cpu", _order=None)
    vars(stub).update(kw)
    stub._pass_frame = lambda name, who=None: DeferredPasses._pass_frame(stub, name, who)
    return stub, lambda *a, **k: DeferredPasses.contour_edges(stub, *a, **k)


def test_contour_edges_refuses_bad_arguments_before_it_looks_at_the_device():
    """The checks of the Python layer on a stand-in that has no device at all (and no library: nothing is launched)."""
    import torch
    stub, contour_edges = _stub()
    table = np.full((5, 3), -1, np.int32)
    for bad, word in ((table.astype(np.int64), "int32"), (table[:, :2], r"\(5, 2\)"), (table.reshape(-1), r"\(15,\)"),
                      (table.astype(np.float32), "int32"), (torch.zeros((5, 3), dtype=torch.int16), "int32")):
        with pytest.raises(ValueError, match=word):
            contour_edges(bad)
    with pytest.raises(ValueError, match=r"partner table holds 4 triangles, the last frame drew 5"):
        contour_edges(table[:4])
    for bad, word in ((np.zeros(5, np.int8), "uint8"), (np.zeros((5, 1), np.uint8), r"\(5, 1\)"), (np.zeros(5, bool), "uint8")):
        with pytest.raises(ValueError, match=word):
            contour_edges(table, static=bad)
    with pytest.raises(ValueError, match=r"static mask holds 6 triangles, the last frame drew 5"):
        contour_edges(table, static=np.zeros(6, np.uint8))
    stub, contour_edges = _stub(_inputs=None)
    with pytest.raises(ValueError, match="contour_edges: no frame has been rendered"):
        contour_edges(table)
    stub, contour_edges = _stub(_pipeline=object())
    with pytest.raises(ValueError, match=r"contour_edges is not available on a swap chain \(pipeline=True\)"):
        contour_edges(table)
    # no winner plane is needed (the stand-in has none), and without triangles nothing is launched
    stub, contour_edges = _stub(T=0)
    out = contour_edges(np.zeros((0, 3), np.int32), static=np.zeros(0, np.uint8), borders=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (0,)


class _Mesh:
    """What the Renderer reads off a model for the wire pass."""

    def __init__(self, tri):
        self._vertices_by_triangles = tri


# a filler that records what the Renderer asks of it
_Recorder = recording_filler("render_model set_fused_illumination wire_pass contour_edges phong_pass resolve",
                             returns=dict(contour_edges="view mask", resolve="resolved"), quiet="get_color_tensor")


def test_renderer_builds_the_table_once_and_the_mask_every_frame():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    from cython3dmodelrenderer_amd.wireframe import edge_partners, feature_edges
    tri = contour_ref.place(contour_ref.open_cylinder())
    model = _Mesh(tri)
    opts = dict(contours=True, feature_angle=30, outline=True, fill=(1, 2, 3))
    f = _Recorder()
    r = Renderer(f, GuroIllumination((0.3, -0.2, 1.0)), on_device="fused", wireframe=opts)
    assert r.wireframe == opts and r.wireframe is not opts
    assert r.render(model) == "colour" and r.render(model) == "colour"
    names = [c[0] for c in f.calls]
    assert names == ["set_fused_illumination", "render_model", "contour_edges", "wire_pass"] * 2
    (_, a0, k0), (_, a1, k1) = [c for c in f.calls if c[0] == "contour_edges"]
    assert a0[0] is a1[0] is r._wired[2] and k0["static"] is k1["static"] is r._wired[1]       # once per model
    assert np.array_equal(a0[0], edge_partners(tri)) and np.array_equal(k0["static"], feature_edges(tri, 30))
    assert k0["borders"] is True                                                               # a contour drawing wants its rim
    assert [c[2] for c in f.calls if c[0] == "wire_pass"] == [dict(outline=True, fill=(1, 2, 3), edges="view mask")] * 2
    other = _Mesh(tri.copy())
    r.render(other)
    assert r._wired[0]() is other and f.calls[-2][1][0] is r._wired[2] and f.calls[-2][1][0] is not a0[0]
    # borders off; an explicit mask is the static one; none at all
    explicit = np.full(len(tri), 5, np.uint8)
    for extra, static in ((dict(edges=explicit), explicit), (dict(), None)):
        f = _Recorder(16, 16)
        r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), None, 8, 8, on_device=True, supersample=2,
                     wireframe=dict(contours=True, borders=False, width=2.0, **extra))
        assert r.render(model) == "resolved"
        assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "phong_pass", "contour_edges", "wire_pass",
                                           "resolve"]
        assert f.calls[3][2] == dict(static=static, borders=False) and r._wired[1] is None
        assert f.calls[4] == ("wire_pass", (), dict(width=2.0, edges="view mask"))
    # without "contours" the call is the parent's: no table, no classification
    f = _Recorder()
    r = Renderer(f, GuroIllumination((0.3, -0.2, 1.0)), on_device="fused", wireframe=dict(feature_angle=30, outline=True))
    r.render(model)
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "wire_pass"]
    assert set(f.calls[-1][2]) == {"outline", "edges"} and f.calls[-1][2]["edges"] is r._wired[1] and r._wired[2] is None
    assert np.array_equal(r._wired[1], feature_edges(tri, 30))

    class NoContours:
        wire_pass = None
    with pytest.raises(ValueError, match="has no contour_edges"):
        Renderer(NoContours(), GuroIllumination((0.3, -0.2, 1.0)), wireframe=dict(contours=True))
    Renderer(NoContours(), GuroIllumination((0.3, -0.2, 1.0)), wireframe=dict(feature_angle=30))
