"""The numpy path on the host: the key rule, the BLAS orders it relies on, the random stream, the
iterators, the host filler and Renderer against the reference's fixtures (scripts/make_py_golden.py),
the vectorised model tests/py_ref.py, Buffer and the uint8 Guro."""
import json
import os

import numpy as np
import pytest

from cython3dmodelrenderer_amd import py
from cython3dmodelrenderer_amd.py.data_structures import Buffer
from cython3dmodelrenderer_amd.py.illumination import GuroIllumination, NoIllumination
from cython3dmodelrenderer_amd.py.pixel_buffer_filler import AdvancedPixelBufferFiller
from cython3dmodelrenderer_amd.triangle_iterator import DepthIterator, SimpleIterator, TriangleIterator
from cython3dmodelrenderer_amd import scenes

import py_ref
from pass_scenes import TriangleModel as Soup
from util import sha

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
with open(os.path.join(GOLDEN, "py_golden.json")) as _fh:
    DOC = json.load(_fh)
SOUPS = np.load(os.path.join(GOLDEN, "py_soups.npz"))


def soup(s):
    return SOUPS[f"s{s}_tri"], SOUPS[f"s{s}_col"], SOUPS[f"s{s}_nrm"]


def _blas_order_failures():
    """Which BLAS orders of the contract (include/crender_py.h steps 5 and 7) this numpy breaks."""
    rng = np.random.default_rng(7)
    failed = []
    for n in (1, 2, 3, 5, 17):
        bar = rng.uniform(0, 1, (n, 3))
        l0, l1, l2 = bar.T
        v = rng.uniform(0, 2, (3, 1)).astype(np.float32)           # step 5: [n,3] @ [3,1] float32 z
        z0, z1, z2 = v[:, 0].astype(np.float64)
        want = py_ref.fma(l2, z2, py_ref.fma(l0, z0, l1 * z1)) if n >= 2 else \
            py_ref.fma(l2, z2, py_ref.fma(l1, z1, l0 * z0))
        if not np.array_equal(np.dot(bar, v)[:, 0], want):
            failed.append(f"depth n={n}")
        for vals in (rng.uniform(0, 256, (3, 3)).astype(np.float32), rng.integers(0, 256, (3, 3))):
            got = np.dot(bar, vals.astype(np.float64) if vals.dtype != np.float32 else vals)   # step 7
            w = vals.astype(np.float64)
            want = py_ref.fma(l2[:, None], w[2], py_ref.fma(l1[:, None], w[1], l0[:, None] * w[0]))
            if not np.array_equal(got, want):
                failed.append(f"attributes n={n} {vals.dtype}")
    return failed


BLAS_FAILURES = _blas_order_failures()


def _blas_orders_hold():
    return not BLAS_FAILURES


LIVE_BLAS = _blas_orders_hold()
live_blas = pytest.mark.skipif(not LIVE_BLAS, reason="LOUD: this numpy's BLAS sums the depth or attribute "
                               "dots in another order than the fixtures' (OpenBLAS 0.3.29, Haswell kernels): "
                               "live-numpy comparisons skipped, fixture comparisons still run")


# ---------------------------------------------------------------- the key rule --
def test_key_rule_matches_the_sequential_depth_test():
    rng = np.random.default_rng(11)
    for case in range(20000):
        k = int(rng.integers(1, 7))
        base = rng.uniform(0, 1)
        ulp = np.spacing(np.float32(base))
        z = base + rng.integers(-2, 3, k) * ulp * rng.choice([0.5, 1.0, 0.25], k)
        if rng.integers(4) == 0:
            z[:] = rng.choice([0.0, -0.0], k)
        s0 = rng.choice([np.float32(1e6), np.float32(base), np.float32(z[0]), np.float32(-0.0)])
        # sequential
        s = np.float32(s0)
        win = 0
        for i, zi in enumerate(z):
            if zi < np.float64(s):
                s, win = np.float32(zi), i + 1
        # keys
        keys = [int(py_ref.ordered(np.float32(s0))) << 32 | (1 << 31)]
        for i, zi in enumerate(z):
            zf = np.float32(zi)
            lo = (py_ref.TIE_MAX - (i + 1)) if zi < np.float64(zf) else ((1 << 31) | (i + 1))
            keys.append(int(py_ref.ordered(zf)) << 32 | lo)
        assert int(np.argmin(keys)) == win, (case, z, s0)


def test_emulated_fma_is_exact():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.uniform(-2, 2, 3000) * 2.0 ** rng.integers(-30, 10, 3000)
    b = rng.uniform(-300, 300, 3000).astype(np.float32).astype(np.float64)
    c = rng.uniform(-2, 2, 3000) * 2.0 ** rng.integers(-30, 10, 3000)
    got = py_ref.fma(a, b, c)
    for i in range(3000):
        assert got[i] == float(Fraction(a[i]) * Fraction(b[i]) + Fraction(c[i])), i


def test_blas_order_guard():
    """The depth and attribute dot orders the device reproduces, probed on this numpy: a mismatch skips
    (loudly, naming the orders) every comparison against live numpy; the fixture comparisons still run."""
    if BLAS_FAILURES:
        pytest.skip("LOUD: this numpy's BLAS breaks the fixtures' orders: " + ", ".join(BLAS_FAILURES))


def test_tiny_negative_normal_sum_is_culled_like_the_reference():
    """A z sum of -2^-149 has a float32 mean of -0, which the reference culls (np.dot >= 0)."""
    nrm = np.zeros((1, 3, 3), np.float32)
    nrm[0, 0, 2] = -np.float32(2.0 ** -149)
    assert np.dot([0, 0, 1], np.mean(nrm[0], axis=0)) >= 0               # the reference's test
    tri = np.float32([[[-0.5, -0.5, 1], [0.5, -0.5, 1], [0, 0.5, 1]]])
    col = np.full((1, 3, 3), 200, np.float32)
    z, c, n = py_ref.new_planes(16, 16)
    py_ref.draw(tri, col, nrm, z, c, n, 90.0)
    assert (z == np.float32(1e6)).all()
    filler = AdvancedPixelBufferFiller(16, 16)
    zb, cb, nb = Buffer(16, 16, 1, init_val=1e6), Buffer(16, 16, 3, "uint8"), Buffer(16, 16, 3)
    filler.compute_triangle_statistics(tri[0], col[0], nrm[0], cb, zb, nb)
    assert (zb[...] == np.float32(1e6)).all()
    nrm[0, 1, 2] = -np.float32(2.0 ** -149)                              # -2^-148: a mean of -2^-149, drawn
    py_ref.draw(tri, col, nrm, z, c, n, 90.0)
    assert (z < 1e6).sum() > 20


def test_random_colour_stream_equivalence():
    np.random.seed(99)
    one = np.random.randint(256, size=(5000, 3))
    after_one = np.random.randint(1 << 30)
    np.random.seed(99)
    many = np.stack([np.random.randint(256, size=3) for _ in range(5000)])
    after_many = np.random.randint(1 << 30)
    assert np.array_equal(one, many) and after_one == after_many


# ------------------------------------------------------------------ iterators --
@pytest.mark.parametrize("s", range(4))
@pytest.mark.parametrize("name,it", [("simple", SimpleIterator), ("depth", DepthIterator)])
def test_iterator_orders_match_the_reference(s, name, it):
    tri, col, nrm = soup(s)
    want = SOUPS[f"s{s}_{name}_order"]
    m = Soup(tri, col, nrm)
    got = [next(i for i in range(len(tri)) if np.shares_memory(t[0], tri[i])) for t in it(m)]
    assert np.array_equal(got, want)
    order = it.draw_order(m)
    assert np.array_equal(np.arange(len(tri)) if order is None else order, want)
    assert issubclass(it, TriangleIterator) and len(it(m)) == len(tri)
    assert list(it(m)) and iter(it(m)) is not None
    with pytest.raises(StopIteration):
        exhausted = it(m)
        for _ in range(len(tri) + 1):
            next(exhausted)


# --------------------------------------------------- host filler and Renderer --
def host_render(s, it):
    tri, col, nrm = soup(s)
    filler = AdvancedPixelBufferFiller(DOC["soups"]["h"], DOC["soups"]["w"], fov=DOC["soups"]["fov"])
    r = py.Renderer(filler, NoIllumination(), it, *filler.get_size(), use_tqdm=False)
    r.pixel_buffer_filler = _HostOnly(filler)
    r.render(Soup(tri, col, nrm))
    return r


class _HostOnly:
    """The filler without its device draw: the Renderer takes the per-triangle loop."""

    def __init__(self, f):
        self.compute_triangle_statistics = f.compute_triangle_statistics


@live_blas
@pytest.mark.parametrize("s", range(4))
@pytest.mark.parametrize("name,it", [("simple", SimpleIterator), ("depth", DepthIterator)])
def test_host_filler_soups_match_fixtures(s, name, it):
    r = host_render(s, it)
    for plane, buf in (("z", r.z_buffer), ("color", r.color_buffer), ("normals", r.n_buffer)):
        assert np.array_equal(buf.get_image().view(np.uint8), SOUPS[f"s{s}_{name}_{plane}"].view(np.uint8)), plane


@live_blas
def test_host_renderer_cube_matches_fixture():
    tri, col, nrm = scenes.load_fixture("cube_inputs.npz")
    sc = DOC["scenes"]["cube256"]
    filler = AdvancedPixelBufferFiller(sc["h"], sc["w"], fov=DOC["fov"])
    r = py.Renderer(_HostOnly(filler), NoIllumination(), SimpleIterator, sc["h"], sc["w"], use_tqdm=False)
    np.random.seed(DOC["seed"])
    r.render(Soup(tri, None, nrm))
    want = sc["cases"]["simple_random"]
    assert sha(r.z_buffer.get_image()) == want["z"]
    assert sha(r.color_buffer.get_image()) == want["color"]
    assert sha(r.n_buffer.get_image()) == want["normals"]
    GuroIllumination([0, 0, 1]).draw_illumination(r.color_buffer, r.n_buffer)
    assert sha(r.color_buffer.get_image()) == want["guro_color"]


@pytest.mark.parametrize("s", range(4))
@pytest.mark.parametrize("name,it", [("simple", SimpleIterator), ("depth", DepthIterator)])
def test_py_ref_soups_match_fixtures(s, name, it):
    tri, col, nrm = soup(s)
    order = it.draw_order(Soup(tri, col, nrm))
    if order is not None:
        tri, col, nrm = tri[order], col[order], nrm[order]
    z, c, n = py_ref.new_planes(DOC["soups"]["h"], DOC["soups"]["w"])
    py_ref.draw(tri, col, nrm, z, c, n, DOC["soups"]["fov"])
    for plane, got in (("z", z), ("color", c), ("normals", n)):
        assert np.array_equal(got.view(np.uint8), SOUPS[f"s{s}_{name}_{plane}"].view(np.uint8)), plane


@pytest.mark.parametrize("scene,case", [("cube256", "simple_own"), ("trex1024", "depth_own"),
                                        ("trex1024", "simple_white")])
def test_py_ref_scenes_match_fixtures(scene, case):
    sc = DOC["scenes"][scene]
    tri, col, nrm = scenes.load_fixture(sc["fixture"])
    if case.startswith("depth"):
        order = DepthIterator.draw_order(Soup(tri, col, nrm))
        tri, col, nrm = tri[order], col[order], nrm[order]
    if case.endswith("white"):
        col = np.full_like(col, 255)
    z, c, n = py_ref.new_planes(sc["h"], sc["w"])
    py_ref.draw(tri, col, nrm, z, c, n, DOC["fov"])
    want = sc["cases"][case]
    assert (sha(z), sha(c), sha(n)) == (want["z"], want["color"], want["normals"])


# ---------------------------------------------------------- Buffer and Guro --
def test_buffer_semantics_and_write_to_file(tmp_path):
    from PIL import Image
    b = Buffer(4, 5, dim=3, dtype="uint8")
    assert b.get_size() == (4, 5) and b.get_image().shape == (4, 5, 3) and b[...].sum() == 0
    b.set_pixel(1, 2, [10, 20, 30])
    b.set_pixel(7, 2, [1, 1, 1])                  # off the buffer: ignored
    b[0, 0] = [200, 100, 50]
    assert list(b.get_pixel(1, 2)) == [10, 20, 30] and b.get_image().sum() == 410
    path = str(tmp_path / "out.png")
    b.write_to_file(path)
    img = np.asarray(Image.open(path))             # RGB of the flipped rows
    assert np.array_equal(img, b.get_image()[::-1][..., ::-1])
    z = Buffer(2, 3, dim=1, init_val=1e6)
    assert z.get_image().dtype == np.float32 and (z[...] == np.float32(1e6)).all()
    z[0, 0] = 0.5
    z.clear()
    assert (z[...] == np.float32(1e6)).all()


def test_guro_uint8():
    rng = np.random.default_rng(5)
    c = Buffer(16, 16, dim=3, dtype="uint8")
    n = Buffer(16, 16, dim=3, dtype="float32")
    c[...] = rng.integers(0, 256, (16, 16, 3))
    n[...] = rng.normal(0, 1, (16, 16, 3)).astype(np.float32)
    n[0, 0] = 0
    before = c[...].copy()
    GuroIllumination([0, 0, 1]).draw_illumination(c, n)
    nb = n[...]
    l = np.array([0, 0, -1], np.float32)
    s = ((np.float32(0) + nb[..., 0] * l[0]) + nb[..., 1] * l[1]) + nb[..., 2] * l[2]
    m = np.sqrt((nb[..., 0] * nb[..., 0] + nb[..., 1] * nb[..., 1]) + nb[..., 2] * nb[..., 2])
    f = np.clip(s / (m + np.float32(1e-6)), 0, 1)[..., None]
    assert np.array_equal(c[...], (before.astype(np.float32) * f).astype(np.uint8))
    assert (c[0, 0] == 0).all()


def test_buffer_set_pixel_drops_what_is_off_the_plane():
    b = Buffer(3, 4, dim=1, dtype="float32")
    for x, y in ((-1, 0), (4, 0), (0, 3), (1.5, 1), (np.nan, 1), ("a", 0)):
        b.set_pixel(x, y, 9)
    assert b[...].sum() == 0
    b.set_pixel(np.int64(3), 2, 7)
    assert b.get_pixel(3, 2)[0] == 7
    u = Buffer(2, 2, dim=3, dtype="uint8", init_val=5)
    assert (u[...] == 5).all() and u[...].dtype == np.uint8
