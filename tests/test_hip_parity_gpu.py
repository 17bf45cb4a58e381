"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle on the
same inputs.  Bar: bit-exact for everything (float32 z / colour / normal planes compared
as uint32, winner-triangle plane as int32) — stricter than north_star's 1e-5 for floats,
because colours reach 255 where 1 ulp = 1.5e-5."""
import os

import numpy as np
import pytest

from model_ref import plain_f32_vertex_normals as _plain_f32_vertex_normals
from util import assert_bit_equal, numpy_dot3_is_double_accumulated, random_soup, sha

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cython3dmodelrenderer_amd import _capi, lowlevel
    _capi.load()
    return lowlevel


# CRENDER_FUZZ_SOAK=n: n times the seeds of the session fuzz tests (a one-off soak; 1 in the committed runs)
_SOAK = max(1, int(os.environ.get("CRENDER_FUZZ_SOAK", "1")))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def oracle_frame(O, tri, col, nrm, H, W, fov=45.0, strips=None, prior=None):
    f = O.OracleFiller(H, W, fov=fov)
    if prior is not None:
        f.z_buffer[...], f.color_buffer[...], f.normals_buffer[...] = prior
    for (y0, y1) in (strips or [(0, H)]):
        f.render_arrays(tri, col, nrm, y0=y0, y1=y1)
    return f


def gpu_frame(hip, tri, col, nrm, H, W, fov=45.0, mode="fused", tile=0, strips=None, prior=None,
              clear=False, bin_capacity=0, raster_path=None):
    """mode: 'fused' = crender_render_model, 'split' = crender_project + crender_raster,
    'atomic' = crender_project + crender_raster_atomic; 'fused-scan' / 'split-scan' force the
    count / scan / fill binning passes (CRENDER_NO_DIRECT_BINS)."""
    extra = 0
    direct = not mode.endswith("-scan")
    mode = mode.replace("-scan", "")
    P = hip.projection_matrix(fov, 0.1, 1000.0, H, W)
    fb = hip.FrameBuffers(H, W)
    if prior is not None:
        fb.load(*prior)
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    proj = None
    if mode != "fused":
        proj = hip.project(t, P, W, H)
    for (y0, y1) in (strips or [(0, H)]):
        if mode == "atomic":
            hip.raster_atomic(proj, c, n, fb, y0=y0, y1=y1, clear=clear)
            continue
        plan = hip.Plan(H, W, max(len(tri), 1), y0=y0, y1=y1, tile=tile, bin_capacity=bin_capacity)
        if raster_path is not None:
            plan.set_raster_path(raster_path)
        for attempt in range(2):
            if mode == "fused":
                hip.render_model(plan, t, c, n, P, fb, clear=clear, direct_bins=direct, flags=extra)
            else:
                hip.raster(plan, proj, c, n, fb, clear=clear, direct_bins=direct, flags=extra)
            need, cap = plan.bin_usage()
            if need <= cap:
                break
            # only the direct bins may overflow here; the plan has switched itself to the
            # general path and the frame is simply rendered again (exact: per-pixel minimum)
            assert attempt == 0 and plan.last_frame_direct(), (need, cap)
        if raster_path is not None and tile == 32:
            assert plan.last_raster_path() == raster_path
    z, cb, nb, win = fb.numpy()
    return z, cb, nb, win, (proj.cpu().numpy() if proj is not None else None)


def compare(got, f, what, check_winner=True):
    z, cb, nb, win, _ = got
    assert_bit_equal(z, f.z_buffer, f"{what}: z")
    assert_bit_equal(cb, f.color_buffer, f"{what}: colour")
    assert_bit_equal(nb, f.normals_buffer, f"{what}: normal")
    if check_winner:
        assert_bit_equal(win, f.winner, f"{what}: winner triangle")


def scene(name):
    from cython3dmodelrenderer_amd import scenes
    return scenes.load_fixture(name)


# ------------------------------------------------------------------------------------
def test_hip_library_is_the_loaded_one(hip):
    from cython3dmodelrenderer_amd import _capi
    with open("/proc/self/maps") as fh:
        assert os.path.realpath(_capi.lib_path()) in fh.read()


@pytest.mark.parametrize("fov,h,w", [(45.0, 1024, 1024), (90.0, 512, 512), (60.0, 300, 500),
                                     (33.3, 4096, 2048)])
def test_projection_matrix(hip, oracle, fov, h, w):
    assert_bit_equal(hip.projection_matrix(fov, 0.1, 1000.0, h, w),
                     oracle.projection_matrix(fov, 0.1, 1000.0, h, w), "proj_mat")
    assert_bit_equal(hip.projection_matrix(fov, 0.5, 50.0, h, w),
                     oracle.projection_matrix(fov, 0.5, 50.0, h, w), "proj_mat")


@pytest.mark.parametrize("T", [1, 3, 255, 256, 257, 1000, 13814])
def test_project_bit_exact(hip, oracle, T):
    rng = np.random.default_rng(T)
    tri = rng.uniform(-2, 2, (T, 3, 3)).astype(np.float32)
    tri[..., 2] = rng.uniform(0.05, 5, (T, 3)).astype(np.float32)
    if T > 8:
        tri[1, 0, 2] = -0.7                       # behind the camera: processed silently
        tri[2, 1, 2] = 1e-30                      # tiny z -> huge / inf coordinates
        tri[3, 2] = [1e-42, -1e-42, 0.3]          # denormal inputs
        tri[4, 0] = [3e38, -3e38, 2.0]            # overflow in the products
        tri[5, 1, 2] = np.float32(np.inf)
    P = oracle.projection_matrix(45.0, 0.1, 1000.0, 720, 1280)
    want = oracle.project(tri, P, 1280, 720)
    t = _dev(tri)
    got = hip.project(t, P, 1280, 720).cpu().numpy()
    m = ~np.isnan(want)
    assert (np.isnan(got) == ~m).all()
    assert_bit_equal(got[m], want[m], "projected")
    hip.project(t, P, 1280, 720, out=t)           # in place, as the reference does (.pyx:99)
    assert_bit_equal(t.cpu().numpy()[m], want[m], "projected in place")


def test_project_trex_matches_golden(hip, oracle, golden):
    tri, _, _ = scene("trex_inputs.npz")
    P = oracle.projection_matrix(45.0, 0.1, 1000.0, 1024, 1024)
    got = hip.project(_dev(tri), P, 1024, 1024).cpu().numpy()
    assert sha(got) == golden["scenes"]["trex1024"]["proj"]


SCENES = [("cube64", "cube_inputs.npz", 64), ("cube256", "cube_inputs.npz", 256),
          ("trex128", "trex_inputs.npz", 128), ("trex256", "trex_inputs.npz", 256),
          ("trex1024", "trex_inputs.npz", 1024), ("bunny512", "bunny_inputs.npz", 512)]


@pytest.mark.parametrize("name,fixture,res", SCENES)
@pytest.mark.parametrize("mode,tile", [("fused", 16), ("fused", 32), ("fused", 64), ("fused-scan", 16),
                                       ("fused-scan", 32), ("split", 0), ("split-scan", 0), ("atomic", 0)])
def test_scenes_match_oracle_and_golden(hip, oracle, golden, name, fixture, res, mode, tile):
    tri, col, nrm = scene(fixture)
    f = oracle_frame(oracle, tri, col, nrm, res, res)
    got = gpu_frame(hip, tri, col, nrm, res, res, mode=mode, tile=tile)
    compare(got, f, f"{name}/{mode}/{tile}")
    g = golden["scenes"][name]
    assert (sha(got[0]), sha(got[1]), sha(got[2]), sha(got[3])) == (g["z"], g["c"], g["n"], g["winner"])
    if got[4] is not None:
        assert sha(got[4]) == g["proj"]


@pytest.mark.parametrize("mode", ["fused", "atomic"])
def test_fused_clear_equals_clear_then_render(hip, oracle, mode):
    tri, col, nrm = scene("trex_inputs.npz")
    f = oracle_frame(oracle, tri, col, nrm, 256, 256)
    rng = np.random.default_rng(0)
    junk = (rng.uniform(-1, 2, (256, 256)).astype(np.float32),
            rng.uniform(0, 255, (256, 256, 3)).astype(np.float32),
            rng.standard_normal((256, 256, 3)).astype(np.float32))
    got = gpu_frame(hip, tri, col, nrm, 256, 256, mode=mode, prior=junk, clear=True)
    compare(got, f, f"fused clear/{mode}")


@pytest.mark.parametrize("mode,tile", [("fused", 16), ("fused", 32), ("fused", 64), ("fused-scan", 32),
                                       ("atomic", 0)])
def test_buffers_composite_across_calls(hip, oracle, mode, tile):
    """The reference never clears: a second render_model draws on top.
    The prior plane also holds values EQUAL to incoming fragments (they must be overwritten)
    and NaN / inf entries."""
    rng = np.random.default_rng(11)
    H, W = 160, 224
    a = random_soup(rng, 400, 200, size_px=(5, 60))
    b = random_soup(rng, 300, 200, size_px=(2, 25))
    first = oracle_frame(oracle, *a, H, W)
    prior = (first.z_buffer.copy(), first.color_buffer.copy(), first.normals_buffer.copy())
    prior[0][5, 7] = np.nan
    prior[0][9, 9] = np.inf
    prior[0][11, 3] = -np.inf
    # second call with the SAME triangles plus new ones: every old fragment ties with the prior z
    tri = np.concatenate([a[0], b[0]]); col = np.concatenate([a[1] * 0.5, b[1]]); nrm = np.concatenate([a[2], b[2]])
    f = oracle_frame(oracle, tri, col, nrm, H, W, prior=tuple(p.copy() for p in prior))
    got = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=tile, prior=prior)
    zw, zg = f.z_buffer, got[0]
    nan = np.isnan(zw)
    assert (np.isnan(zg) == nan).all()
    assert_bit_equal(zg[~nan], zw[~nan], "z")
    assert_bit_equal(got[1], f.color_buffer, "colour")
    assert_bit_equal(got[2], f.normals_buffer, "normal")
    touched = f.winner >= 0
    assert_bit_equal(got[3][touched], f.winner[touched], "winner")


@pytest.mark.parametrize("mode,tile", [("fused", 16), ("fused", 32), ("fused", 64), ("fused-scan", 32),
                                       ("atomic", 0)])
def test_row_strips_tile_the_frame(hip, oracle, mode, tile):
    tri, col, nrm = scene("trex_inputs.npz")
    H, W = 300, 260
    f = oracle_frame(oracle, tri, col, nrm, H, W)
    strips = [(0, 37), (37, 101), (101, 128), (128, 300)]
    got = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=tile, strips=strips)
    compare(got, f, f"strips/{mode}")
    # one strip alone touches nothing outside its rows
    got1 = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=tile, strips=[(101, 128)])
    f1 = oracle_frame(oracle, tri, col, nrm, H, W, strips=[(101, 128)])
    compare(got1, f1, f"single strip/{mode}")
    assert (got1[0][:101] == 1e6).all() and (got1[0][128:] == 1e6).all()


@pytest.mark.parametrize("seed,T,H,W,px,kw", [
    (1, 1, 64, 64, (10, 30), {}),
    (2, 37, 97, 131, (1, 6), {}),                     # odd sizes, not a multiple of the tile
    (3, 5000, 256, 256, (0.3, 4), {}),                # tiny: many empty pixel boxes
    (4, 20000, 512, 384, (1, 12), {}),
    (5, 300, 512, 512, (100, 600), {}),               # huge: span many tiles, clipped by the frame
    (6, 3000, 333, 517, (0.5, 200), {"margin": 1.0}), # mixed sizes, many off-screen
    (7, 60000, 1024, 1024, (1, 9), {}),
])
@pytest.mark.parametrize("mode,tile", [("fused", 16), ("fused", 32), ("fused", 64), ("fused-scan", 32),
                                       ("atomic", 0)])
def test_random_triangle_soups(hip, oracle, seed, T, H, W, px, kw, mode, tile):
    rng = np.random.default_rng(seed)
    tri, col, nrm = random_soup(rng, T, max(H, W), size_px=px, **kw)
    f = oracle_frame(oracle, tri, col, nrm, H, W)
    got = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=tile)
    compare(got, f, f"soup{seed}/{mode}/{tile}")


@pytest.mark.parametrize("H,W,fov,zn,zf", [(480, 640, 90.0, 0.1, 1000.0), (640, 480, 60.0, 0.5, 50.0),
                                           (1, 1, 45.0, 0.1, 1000.0), (1, 17, 45.0, 0.1, 1000.0),
                                           (17, 1, 45.0, 0.1, 1000.0), (3, 65535, 45.0, 0.1, 1000.0),
                                           (5000, 8, 30.0, 0.01, 10.0), (33, 47, 120.0, 0.1, 1000.0)])
@pytest.mark.parametrize("mode", ["fused", "fused-scan", "atomic"])
def test_frame_shapes_and_camera_parameters(hip, oracle, H, W, fov, zn, zf, mode):
    """Non-square and degenerate frame shapes (1 pixel, single row / column, the 65535 limit),
    non-default fov / z_near / z_far: the projection matrix and the aspect ratio enter K1."""
    rng = np.random.default_rng(H * 7 + W)
    tri, col, nrm = random_soup(rng, 800, max(H, W, 64), size_px=(1, 60), margin=0.5)
    tri[..., :2] *= np.float32(2.4142137 * np.tan(np.radians(fov / 2)))   # fill this frustum
    P = oracle.projection_matrix(fov, zn, zf, H, W)
    f = oracle.OracleFiller(H, W, fov=fov, z_near=zn, z_far=zf)
    assert_bit_equal(f.proj_mat, P, "oracle proj")
    f.render_arrays(tri, col, nrm)
    # gpu_frame builds its matrix with z_near 0.1 / z_far 1000: go through the low-level calls
    fb = hip.FrameBuffers(H, W)
    Pg = hip.projection_matrix(fov, zn, zf, H, W)
    assert_bit_equal(Pg, P, "proj_mat")
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    if mode == "atomic":
        hip.raster_atomic(hip.project(t, Pg, W, H), c, n, fb)
    else:
        plan = hip.Plan(H, W, len(tri))
        for attempt in range(2):
            hip.render_model(plan, t, c, n, Pg, fb, direct_bins=(mode == "fused"))
            need, cap = plan.bin_usage()
            if need <= cap:
                break
            assert attempt == 0 and plan.last_frame_direct()
    compare(tuple(fb.numpy()) + (None,), f, f"{H}x{W} fov {fov} {mode}")


@pytest.mark.parametrize("T", [65535, 65536, 65537])
def test_direct_bin_triangle_limit(hip, oracle, T):
    """Scenes of up to 65536 triangles use the direct bins (48-byte entries, binning mode 1), larger ones
    the pair bins (one pass into per-tile slabs of (position, index) pairs, mode 2) — or, when asked
    (CRENDER_NO_DIRECT_BINS), the count / scan / fill passes (mode 0)."""
    rng = np.random.default_rng(T)
    tri, col, nrm = random_soup(rng, T, 512, size_px=(0.5, 5))
    f = oracle_frame(oracle, tri, col, nrm, 384, 512)
    P = hip.projection_matrix(45.0, 0.1, 1000.0, 384, 512)
    fb = hip.FrameBuffers(384, 512)
    plan = hip.Plan(384, 512, T)
    hip.render_model(plan, _dev(tri), _dev(col), _dev(nrm), P, fb)
    assert plan.last_frame_direct() and plan.last_frame_binning() == (1 if T <= 65536 else 2)
    need, cap = plan.bin_usage()
    assert need <= cap
    compare(tuple(fb.numpy()) + (None,), f, f"T={T}")
    fb2 = hip.FrameBuffers(384, 512)
    hip.render_model(plan, _dev(tri), _dev(col), _dev(nrm), P, fb2, direct_bins=False)
    assert not plan.last_frame_direct() and plan.last_frame_binning() == 0
    compare(tuple(fb2.numpy()) + (None,), f, f"T={T}, scan path")


@pytest.mark.parametrize("mode,tile", [("fused", 16), ("fused", 32), ("fused", 64), ("fused-scan", 32),
                                       ("atomic", 0)])
def test_adversarial_triangles(hip, oracle, mode, tile):
    """Edge cases of SURVEY.md section 7 step 1: exact ties (duplicates and a shared edge), zero-area
    triangles (l3 = 0 -> inf/NaN barycentrics), vertices exactly on pixel centres, triangles
    fully / partly off screen, a vertex behind the camera, NaN / inf coordinates, -0 depths."""
    rng = np.random.default_rng(99)
    H = W = 128
    tri, col, nrm = random_soup(rng, 64, 128, size_px=(8, 50), frac_backface=0.0)
    extra = []
    quad = np.array([[-0.2, -0.2, 1.0], [0.2, -0.2, 1.0], [0.2, 0.2, 1.0], [-0.2, 0.2, 1.0]], np.float32)
    extra += [quad[[0, 1, 2]], quad[[0, 2, 3]]]                      # shared diagonal
    extra += [tri[5].copy(), tri[5].copy(), tri[9].copy()]           # duplicates -> ties
    deg = tri[3].copy(); deg[2] = deg[0]; extra.append(deg)           # zero area
    line = tri[4].copy(); line[2] = (line[0] + line[1]) / 2; extra.append(line)
    extra.append(np.array([[5, 5, 1], [6, 5, 1], [5, 6, 1]], np.float32))      # off screen
    behind = tri[6].copy(); behind[1, 2] = -0.5; extra.append(behind)
    nanv = tri[7].copy(); nanv[0, 0] = np.nan; extra.append(nanv)
    infv = tri[8].copy(); infv[2, 1] = np.inf; extra.append(infv)
    # vertices that project exactly onto integer pixels (x = 32, 64, 96 at z = 1)
    f0 = 2.4142137
    on = np.array([[(32 / 64 - 1) / f0, (32 / 64 - 1) / f0, 1.0], [(96 / 64 - 1) / f0, (32 / 64 - 1) / f0, 1.0],
                   [(64 / 64 - 1) / f0, (96 / 64 - 1) / f0, 1.0]], np.float32)
    extra.append(on)
    extra = np.stack(extra)
    tri = np.concatenate([tri, extra])
    col = np.concatenate([col, rng.uniform(0, 255, extra.shape).astype(np.float32)])
    n_extra = rng.standard_normal(extra.shape).astype(np.float32)
    n_extra[..., 2] = -np.abs(n_extra[..., 2])
    nrm = np.concatenate([nrm, n_extra])
    nrm[10, :, 2] = [0.0, -0.0, 0.0]          # sum == +0 -> culled (>= 0)
    nrm[11, :, 2] = [1e-45, -1e-45, -1e-45]   # denormal negative sum -> drawn
    f = oracle_frame(oracle, tri, col, nrm, H, W)
    got = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=tile)
    compare(got, f, f"adversarial/{mode}/{tile}")
    assert (f.winner >= 0).sum() > 1000


@pytest.mark.parametrize("mode,tile", [("fused", 16), ("fused", 32), ("fused-scan", 32), ("fused", 64),
                                       ("atomic", 0)])
def test_adversarial_large_triangles(hip, oracle, mode, tile):
    """The large-record sweep (coarse block cull + survivor masks) on awkward input: slivers a
    fraction of a pixel wide but hundreds long, zero-area and collinear triangles, duplicates
    (exact z ties), vertices far off screen, a vertex behind the camera, NaN / inf coordinates,
    all large enough that batches average >= 16 blocks per record."""
    rng = np.random.default_rng(123)
    H, W = 200, 264
    tri, col, nrm = random_soup(rng, 24, 256, size_px=(150, 700), frac_backface=0.0, margin=0.6)
    extra = []
    for k in range(6):                                   # slivers: two vertices almost coincide
        t = tri[k].copy(); t[1] = t[0] + np.float32(1e-3) * (k + 1); extra.append(t)
    t = tri[6].copy(); t[2] = t[0]; extra.append(t)       # zero area
    t = tri[7].copy(); t[2] = (t[0] + t[1]) / 2; extra.append(t)   # collinear
    extra += [tri[8].copy(), tri[8].copy(), tri[9].copy()]           # duplicates
    t = tri[10].copy(); t[0, :2] *= 40; extra.append(t)   # a vertex far off screen
    t = tri[11].copy(); t[1, 2] = -0.4; extra.append(t)   # behind the camera
    t = tri[12].copy(); t[2, 0] = np.nan; extra.append(t)
    t = tri[13].copy(); t[0, 1] = np.inf; extra.append(t)
    t = tri[14].copy(); t[:, 2] = 1e-3; extra.append(t)   # very close: huge coordinates
    extra = np.stack(extra)
    tri = np.concatenate([tri, extra])
    col = np.concatenate([col, rng.uniform(0, 255, extra.shape).astype(np.float32)])
    ne = rng.standard_normal(extra.shape).astype(np.float32); ne[..., 2] = -np.abs(ne[..., 2])
    nrm = np.concatenate([nrm, ne])
    f = oracle_frame(oracle, tri, col, nrm, H, W)
    got = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=tile)
    compare(got, f, f"adversarial large/{mode}/{tile}")
    assert (f.winner >= 0).mean() > 0.5


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_random_configurations(hip, oracle, seed):
    """Seeded fuzz over everything at once: frame shape, camera, triangle count and size mix,
    tile size, binning path, row strips, compositing on top of a previous frame, fused clear."""
    rng = np.random.default_rng(1000 + seed)
    H = int(rng.integers(1, 400)); W = int(rng.integers(1, 400))
    if seed % 5 == 0:
        H, W = int(rng.integers(500, 1100)), int(rng.integers(500, 1100))
    fov = float(rng.choice([30.0, 45.0, 60.0, 90.0, 110.0]))
    T = int(rng.choice([0, 1, 2, 17, 300, 2500, 9000]))
    lo = float(rng.choice([0.2, 1.0, 4.0])); hi = lo * float(rng.choice([2.0, 10.0, 80.0]))
    tri, col, nrm = random_soup(rng, T, max(H, W, 32), size_px=(lo, hi),
                                margin=float(rng.choice([0.0, 0.5, 1.5])))
    tri[..., :2] *= np.float32(2.4142137 * np.tan(np.radians(fov / 2)))
    tile = int(rng.choice([0, 16, 32, 64]))
    mode = str(rng.choice(["fused", "fused-scan", "split", "atomic"]))
    clear = bool(rng.integers(0, 2))
    prior = None
    if rng.integers(0, 2):
        prior = (rng.uniform(0.2, 3.0, (H, W)).astype(np.float32),
                 rng.uniform(0, 255, (H, W, 3)).astype(np.float32),
                 rng.standard_normal((H, W, 3)).astype(np.float32))
    cuts = sorted(set(int(v) for v in rng.integers(0, H + 1, int(rng.integers(0, 4)))) | {0, H})
    strips = [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]
    zn, zf = 0.1, 1000.0
    f = oracle.OracleFiller(H, W, fov=fov, z_near=zn, z_far=zf)
    if prior is not None and not clear:
        f.z_buffer[...], f.color_buffer[...], f.normals_buffer[...] = prior
    for (y0, y1) in strips:
        f.render_arrays(tri, col, nrm, y0=y0, y1=y1)
    got = gpu_frame(hip, tri, col, nrm, H, W, fov=fov, mode=mode, tile=tile, strips=strips,
                    prior=prior, clear=clear)
    what = f"fuzz {seed}: {H}x{W} fov {fov} T {T} px ({lo},{hi}) tile {tile} {mode} clear {clear} strips {strips}"
    assert_bit_equal(got[0], f.z_buffer, what + ": z")
    assert_bit_equal(got[1], f.color_buffer, what + ": colour")
    assert_bit_equal(got[2], f.normals_buffer, what + ": normal")
    touched = f.winner >= 0
    assert_bit_equal(got[3][touched], f.winner[touched], what + ": winner")


@pytest.mark.parametrize("seed", range(40 * _SOAK))
def test_fuzz_many_frames_on_the_same_plans(hip, oracle, seed):
    """Seeded fuzz over what a plan CARRIES from frame to frame — counter parities, the split tiles' flag and
    helper-slot words, the dispatch-order hint, sticky overflow switches, bins filled and never drawn: one set
    of plans (the whole frame, or two or three row strips), twenty-odd frames of scenes drawn at random from
    a pool (T-Rex, the cube, soups of small / large / very many triangles, no triangles), each through a
    randomly chosen entry point — render_model, project + raster, prepare + draw, prepare TWICE (the first
    binning discarded) + draw — with or without the direct bins, with or without fused clear; after every
    frame the buffers are the oracle's, which was fed the same sequence.  Even seeds: plans for at most
    20 000 triangles (direct bins: small frames are split and ordered); odd seeds: plans for 90 000 (pair
    bins, scan path on request)."""
    import torch
    rng = np.random.default_rng(7000 + seed)
    big_family = seed % 2 == 1
    H = int(rng.choice([256, 384, 512, 700, 1024])); W = int(rng.choice([256, 512, 640, 1024]))
    tile = int(rng.choice([0, 16, 32, 32, 64]))
    fov = 45.0
    pool = {"trex": scene("trex_inputs.npz"), "cube": scene("cube_inputs.npz"),
            "small": random_soup(rng, 3000, max(H, W), size_px=(1, 10)),
            "large": random_soup(rng, 80, max(H, W), size_px=(20, 120)),
            "none": tuple(np.zeros((0, 3, 3), np.float32) for _ in range(3))}
    if big_family:
        pool["many"] = random_soup(rng, 90_000, max(H, W), size_px=(0.5, 4))
    maxT = max(len(v[0]) for v in pool.values())
    dev = {k: [_dev(a) for a in v] for k, v in pool.items()}
    cuts = sorted(set(int(v) for v in rng.integers(1, H, int(rng.integers(0, 3)))) | {0, H})
    strips = [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]
    plans = [hip.Plan(H, W, maxT, y0=a, y1=b, tile=tile) for a, b in strips]
    fb = hip.FrameBuffers(H, W)
    ref = oracle.OracleFiller(H, W, fov=fov)
    P = hip.projection_matrix(fov, 0.1, 1000.0, H, W)
    names = list(pool)
    history = []
    for k in range(22):
        name = names[int(rng.integers(0, len(names)))]
        how = str(rng.choice(["fused", "fused", "split", "prepare+draw", "prepare twice"]))
        direct = bool(rng.integers(0, 4) > 0)
        clear = bool(rng.integers(0, 2))
        other = names[int(rng.integers(0, len(names)))]
        history.append((name, how, direct, clear))
        t, c, n = dev[name]
        T = t.shape[0]
        if clear:
            ref.clear()
        for (a, b) in strips:
            ref.render_arrays(*pool[name], y0=a, y1=b)
        proj = hip.project(t, P, W, H) if how == "split" and T else None
        for plan in plans:
            for attempt in range(2):
                if how == "fused" or T == 0:
                    hip.render_model(plan, t, c, n, P, fb, clear=clear, direct_bins=direct)
                elif how == "split":
                    hip.raster(plan, proj, c, n, fb, clear=clear, direct_bins=direct)
                else:
                    if how == "prepare twice" and dev[other][0].shape[0]:
                        hip.prepare(plan, dev[other][0], dev[other][2], P, direct_bins=direct)   # never drawn
                    hip.prepare(plan, t, n, P, direct_bins=direct)
                    if k % 3 == 0:
                        plan.debug_check()      # binned, not drawn: registrations = flags = helper triples = long lists
                    hip.draw(plan, c, n, T, fb, clear=clear, direct_bins=direct)
                need, cap = plan.bin_usage()
                if need <= cap:
                    break
                assert attempt == 0, (need, cap, history)      # a plan switches to roomier bins once
        z, cb, nb, win = fb.numpy()
        what = f"stateful fuzz {seed}: {H}x{W} tile {tile} strips {strips}, frame {k} of {history}"
        for plan in plans:
            # the state a frame LEAVES, checked as such (crender_plan_debug_check) — before any pixel of a later
            # frame could show it
            try:
                plan.debug_check()
            except Exception as e:
                raise AssertionError(f"{what}: {e}") from e
        assert_bit_equal(z, ref.z_buffer, what + ": z")
        assert_bit_equal(cb, ref.color_buffer, what + ": colour")
        assert_bit_equal(nb, ref.normals_buffer, what + ": normal")
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", range(24 * _SOAK))
def test_fuzz_a_filler_through_a_random_session(oracle, hip, seed):
    """Seeded fuzz of the drop-in CLASS: one AdvancedPixelBufferFiller, forty-odd calls drawn at random —
    render_model on numpy models (composite, as the reference; or clear=True), render_arrays on device
    tensors, bursts of render_frame (with and without the swap chain, depth 1 or the default), clear(),
    getters, in-place edits of the arrays the getters handed out followed by a composite render (the edit
    must be under the new fragments, guro_illumination.py:27 does exactly this), in-place edits of a model's
    vertex array between two render_model calls (.pyx:94-96 re-reads them) — against an oracle filler that is
    told the same story.  Every getter call along the way is compared bit for bit."""
    import torch
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(9000 + seed)
    H = int(rng.choice([200, 256, 512, 640])); W = int(rng.choice([256, 320, 512]))
    kw = {}
    if seed % 3 == 1:
        kw = {"pipeline": True}
    elif seed % 3 == 2:
        kw = {"pipeline": True, "pipeline_depth": 1}
    if rng.integers(0, 2):
        kw["tile"] = int(rng.choice([16, 32]))
    if seed % 4 == 0:
        kw["track_winner"] = True          # (the winner plane must tell the same story)
    strip = (0, H)
    if seed % 5 == 4:
        a = int(rng.integers(0, H // 2)); strip = (a, int(rng.integers(a + 1, H + 1)))
        kw["row_strip"] = strip            # (a filler that owns some rows of the frame only)

    class M:
        def __init__(self, t, c, n):
            self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = t, c, n

    pool = {"trex": scene("trex_inputs.npz"), "cube": scene("cube_inputs.npz"),
            "small": random_soup(rng, 2500, max(H, W), size_px=(1, 9)),
            "large": random_soup(rng, 60, max(H, W), size_px=(20, 110)),
            "none": tuple(np.zeros((0, 3, 3), np.float32) for _ in range(3))}
    if seed % 6 == 5:
        # a model large enough for the filler's tile-coherent snapshot (2^18 triangles: sorted copy, (position,
        # caller's index) pairs in the lists, winners found through the per-tile hash table)
        pool["huge"] = random_soup(rng, 270_000, max(H, W), size_px=(0.5, 3))
    models = {k: M(*(a.copy() for a in v)) for k, v in pool.items()}
    P = hip.projection_matrix(45.0, 0.1, 1000.0, H, W)
    names = list(pool)
    f = AdvancedPixelBufferFiller(H, W, fov=45, **kw)
    ref = oracle.OracleFiller(H, W, fov=45.0)
    views = {}
    story = []

    def ref_clear():                    # (a strip filler clears, and renders, its own rows only)
        a, b = strip
        ref.z_buffer[a:b] = np.float32(1e6); ref.color_buffer[a:b] = 0; ref.normals_buffer[a:b] = 0
        ref.winner[a:b] = -1
    resident = None                     # what render_frame renders: the arrays of the last render call

    def check(what):
        # every plan's cross-frame state (crender_plan_debug_check), which synchronises: before the pixels on even
        # steps, after them on odd ones, where the getters are the first to meet frames in flight and a redo
        if step % 2 == 0:
            f.debug_check()
        for name, get, want in (("z", f.get_z_buffer, ref.z_buffer), ("colour", f.get_color_buffer, ref.color_buffer),
                                ("normal", f.get_normals_buffer, ref.normals_buffer)):
            views[name] = get()
            # (a strip filler answers for its own rows; the others belong to whoever fills them — an exchange)
            assert_bit_equal(views[name][strip[0]:strip[1]], want[strip[0]:strip[1]],
                             f"filler session {seed} ({H}x{W}, {kw}): {what}: {name}; story {story}")
        if kw.get("track_winner"):
            f.synchronize()
            assert_bit_equal(f.get_winner_tensor().cpu().numpy()[strip[0]:strip[1]], ref.winner[strip[0]:strip[1]],
                             f"filler session {seed} ({H}x{W}, {kw}): {what}: winner; story {story}")
        if step % 2:
            f.debug_check()

    fresh = False          # the arrays handed out so far show the buffers: after a getter call, and after every
    #                        render_model, which refreshes them (.pyx:246-253: views of the buffers themselves)
    for step in range(44):
        op = str(rng.choice(["model", "model", "model clear", "arrays", "frames", "projected", "clear", "check",
                             "edit view", "edit view", "edit model"]))
        name = names[int(rng.integers(0, len(names)))]
        story.append((op, name))
        if op == "model" or op == "model clear":
            clear = op == "model clear"
            if clear:
                ref_clear()
            m = models[name]
            ref.render_arrays(m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles, y0=strip[0], y1=strip[1])
            f.render_model(m, clear=clear)
            resident = (m._vertices_by_triangles.copy(), m._colors_by_triangles, m._normals_by_triangles)
            fresh = True
        elif op == "arrays":
            clear = bool(rng.integers(0, 2))
            if clear:
                ref_clear()
            ref.render_arrays(*pool[name], y0=strip[0], y1=strip[1])
            f.render_arrays(*(_dev(a) for a in pool[name]), clear=clear)
            resident = pool[name]
            fresh = False
        elif op == "frames":
            if resident is None:
                continue
            for _ in range(int(rng.integers(1, 6))):
                f.render_frame()
            ref_clear()
            ref.render_arrays(*resident, y0=strip[0], y1=strip[1])
            fresh = False
        elif op == "projected":
            # a frame from ALREADY PROJECTED vertices (K2 alone) with the resident colours and normals
            if resident is None or len(resident[0]) == 0 or f._order is not None:
                continue
            f.render_projected_frame(hip.project(_dev(resident[0]), P, W, H))
            ref_clear()
            ref.render_arrays(*resident, y0=strip[0], y1=strip[1])
            fresh = False
        elif op == "clear":
            f.clear()
            ref_clear()
            fresh = False
        elif op == "check":
            check(f"step {step}")
            fresh = True
        elif op == "edit view":
            # the caller writes into an array a getter handed out; the next render composites on top of it
            if not (fresh and "z" in views and rng.integers(0, 2)):
                check(f"step {step}, before the edit")
            # (else: straight into the arrays a getter handed out EARLIER — they are live)
            y0 = int(rng.integers(strip[0], max(strip[0] + 1, strip[1] - 8))); x0 = int(rng.integers(0, W - 8))
            hh, ww = int(rng.integers(1, 8)), int(rng.integers(1, 8))
            hh = min(hh, strip[1] - y0)
            zval = np.float32(rng.choice([0.3, 0.9, 2.0, 1e6]))
            for v, r in ((views["z"], ref.z_buffer),):
                v[y0:y0 + hh, x0:x0 + ww] = zval
                r[y0:y0 + hh, x0:x0 + ww] = zval
            cval = np.float32(rng.uniform(0, 255))
            views["colour"][y0:y0 + hh, x0:x0 + ww] = cval
            ref.color_buffer[y0:y0 + hh, x0:x0 + ww] = cval
            m = models[name]
            ref.render_arrays(m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles, y0=strip[0], y1=strip[1])
            f.render_model(m)
            resident = (m._vertices_by_triangles.copy(), m._colors_by_triangles, m._normals_by_triangles)
            check(f"step {step}, render on top of the edited arrays")
            fresh = True
        elif op == "edit model":
            m = models[name]
            if len(m._vertices_by_triangles):
                m._vertices_by_triangles[..., 0] += np.float32(rng.uniform(-0.02, 0.02))     # in place
            ref.render_arrays(m._vertices_by_triangles, m._colors_by_triangles, m._normals_by_triangles, y0=strip[0], y1=strip[1])
            f.render_model(m)
            resident = (m._vertices_by_triangles.copy(), m._colors_by_triangles, m._normals_by_triangles)
            fresh = True
    check("the end")
    torch.cuda.synchronize()


@pytest.mark.parametrize("clear", [False, True])
def test_no_triangles(hip, oracle, clear):
    empty = np.zeros((0, 3, 3), np.float32)
    rng = np.random.default_rng(5)
    prior = (rng.uniform(0, 2, (70, 90)).astype(np.float32),
             rng.uniform(0, 255, (70, 90, 3)).astype(np.float32),
             rng.standard_normal((70, 90, 3)).astype(np.float32))
    for mode in ("fused", "atomic"):
        got = gpu_frame(hip, empty, empty, empty, 70, 90, mode=mode, prior=prior, clear=clear)
        if clear:
            assert (got[0] == 1e6).all() and (got[1] == 0).all() and (got[2] == 0).all()
        else:
            assert_bit_equal(got[0], prior[0], "z")
            assert_bit_equal(got[1], prior[1], "colour")
            assert_bit_equal(got[2], prior[2], "normal")


def test_bin_list_overflow_is_reported(hip):
    tri, col, nrm = scene("trex_inputs.npz")
    P = hip.projection_matrix(45.0, 0.1, 1000.0, 512, 512)
    fb = hip.FrameBuffers(512, 512)
    plan = hip.Plan(512, 512, len(tri), bin_capacity=100)
    hip.render_model(plan, _dev(tri), _dev(col), _dev(nrm), P, fb, direct_bins=False)
    need, cap = plan.bin_usage()
    assert cap == 100 and need > cap and not plan.last_frame_direct()
    big = hip.Plan(512, 512, len(tri), bin_capacity=need)
    hip.render_model(big, _dev(tri), _dev(col), _dev(nrm), P, fb, direct_bins=False)
    assert big.bin_usage() == (need, need)


def test_direct_bins_fall_back_when_a_tile_list_overflows(hip, oracle):
    """Small scenes append straight into 1024-entry per-tile lists; 3000 triangles stacked
    in one tile do not fit: the overflow is reported, the plan switches to the general
    path, and the re-rendered frame is exact."""
    rng = np.random.default_rng(8)
    tri, col, nrm = random_soup(rng, 3000, 256, size_px=(2, 6), frac_backface=0.0, margin=-0.9)
    f = oracle_frame(oracle, tri, col, nrm, 256, 256)
    P = hip.projection_matrix(45.0, 0.1, 1000.0, 256, 256)
    fb = hip.FrameBuffers(256, 256)
    plan = hip.Plan(256, 256, len(tri), tile=32)
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    hip.render_model(plan, t, c, n, P, fb)
    assert plan.last_frame_direct()
    need, cap = plan.bin_usage()
    assert cap == 1024 and need > cap
    hip.render_model(plan, t, c, n, P, fb)
    assert not plan.last_frame_direct()
    need, cap = plan.bin_usage()
    assert need <= cap
    compare(tuple(fb.numpy()) + (None,), f, "after direct-bin fallback")


@pytest.mark.parametrize("direct", [True, False])
def test_prepare_and_draw_halves(hip, oracle, direct):
    """crender_prepare + crender_draw == crender_render_model, also with the two halves on
    different streams ordered by an event, and with pre-projected vertices (P16 == NULL)."""
    import torch
    tri, col, nrm = scene("trex_inputs.npz")
    H, W = 240, 320
    f = oracle_frame(oracle, tri, col, nrm, H, W)
    P = hip.projection_matrix(45.0, 0.1, 1000.0, H, W)
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    # same stream
    fb = hip.FrameBuffers(H, W)
    plan = hip.Plan(H, W, len(tri))
    hip.prepare(plan, t, n, P, direct_bins=direct)
    hip.draw(plan, c, n, len(tri), fb, direct_bins=direct)
    assert plan.last_frame_direct() == direct
    compare(tuple(fb.numpy()) + (None,), f, "prepare + draw")
    # two streams, ordered by an event; fused clear over junk
    fb2 = hip.FrameBuffers(H, W)
    fb2.z.fill_(0.5); fb2.color.fill_(7.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    hip.prepare(plan, t, n, P, stream=side, direct_bins=direct)
    done = torch.cuda.Event(); done.record(side)
    torch.cuda.current_stream().wait_event(done)
    hip.draw(plan, c, n, len(tri), fb2, clear=True, direct_bins=direct)
    compare(tuple(fb2.numpy()) + (None,), f, "prepare on a side stream")
    # already projected vertices
    proj = hip.project(t, P, W, H)
    fb3 = hip.FrameBuffers(H, W)
    hip.prepare(plan, proj, n, None, direct_bins=direct)
    hip.draw(plan, c, n, len(tri), fb3, proj=proj, direct_bins=direct)
    compare(tuple(fb3.numpy()) + (None,), f, "pre-projected halves")
    # a draw whose T does not match the prepared frame is refused
    from cython3dmodelrenderer_amd import _capi
    with pytest.raises(_capi.CrenderError):
        hip.draw(plan, c, n, len(tri) - 1, fb3, proj=proj)


def test_c_abi_argument_errors(hip):
    import ctypes as C
    from cython3dmodelrenderer_amd import _capi
    L = _capi.load()
    plan = C.c_void_p()
    assert L.crender_plan_create(C.byref(plan), 64, 64, 10, 5, 10, 0, 0, None, 0, None) == _capi.EINVAL
    assert b"geometry" in L.crender_last_error()
    assert L.crender_plan_workspace_bytes(0, 64, 0, 64, 10, 0, 0) == 0
    assert L.crender_project(None, None, -1, None, 64, 64, None) == _capi.EINVAL
    assert L.crender_clear(None, None, None, None, 64, 64, 0, 64, None) == _capi.EINVAL
    import torch
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda:0")
    assert L.crender_plan_create(C.byref(plan), 64, 64, 0, 64, 1000, 0, 0, ws.data_ptr(), 1024,
                                 None) == _capi.ENOMEM
    # round 6's entry points: the raster kernel choice and the state check
    assert L.crender_plan_set_raster_path(None, 0) == _capi.EINVAL
    assert L.crender_plan_debug_check(None, None, None, 0) == _capi.EINVAL
    assert L.crender_set_default_raster_path(7) == _capi.EINVAL and b"-1" in L.crender_last_error()
    p2 = hip.Plan(64, 64, 10, tile=32)
    assert L.crender_plan_set_raster_path(p2.handle, 2) == _capi.EINVAL
    assert L.crender_plan_set_raster_path(p2.handle, 1) == _capi.OK and L.crender_plan_last_raster_path(p2.handle) == 0
    p2.debug_check()                                  # a plan that has rendered nothing is consistent
    buf = C.create_string_buffer(64)
    assert L.crender_plan_debug_check(p2.handle, None, buf, 64) == _capi.OK and buf.value == b""


def test_fast_division_is_bit_exact(hip):
    """The sweep's division shortcut (raster_math.h (2)) must equal the correctly rounded `/`
    for every operand pair inside its window [2^-40, 2^40]: random mantissas over every
    exponent pair, extreme mantissas, and values straddling the window edges; both are also
    compared with numpy's IEEE division."""
    import torch
    from cython3dmodelrenderer_amd import _capi
    L = _capi.load()
    rng = np.random.default_rng(2024)

    def check(num, den):
        a = torch.from_numpy(num).cuda(); d = torch.from_numpy(den).cuda()
        o1 = torch.empty_like(a); o2 = torch.empty_like(a)
        _capi.check(L.crender_selfcheck_division(a.data_ptr(), d.data_ptr(), o1.data_ptr(),
                                                 o2.data_ptr(), a.numel(), None), "selfcheck")
        torch.cuda.synchronize()
        t, q = o1.cpu().numpy(), o2.cpu().numpy()
        with np.errstate(all="ignore"):
            ref = num / den
        nan = np.isnan(ref)
        assert (np.isnan(t) == nan).all() and (np.isnan(q) == nan).all()
        assert_bit_equal(q[~nan], ref[~nan], "GPU `/` vs numpy")
        assert_bit_equal(t[~nan], q[~nan], "division shortcut vs `/`")

    # (a) every exponent pair of the window (and 3 beyond each edge) x random mantissas + signs
    exps = np.arange(127 - 43, 127 + 44, dtype=np.uint32)
    en, ed = np.meshgrid(exps, exps, indexing="ij")
    reps = 4096
    for chunk in range(8):
        mn = rng.integers(0, 1 << 23, (en.size, reps // 8), dtype=np.uint32)
        md = rng.integers(0, 1 << 23, (en.size, reps // 8), dtype=np.uint32)
        sn = rng.integers(0, 2, mn.shape, dtype=np.uint32) << 31
        sd = rng.integers(0, 2, mn.shape, dtype=np.uint32) << 31
        num = (sn | (en.reshape(-1, 1) << 23) | mn).astype(np.uint32).view(np.float32).ravel()
        den = (sd | (ed.reshape(-1, 1) << 23) | md).astype(np.uint32).view(np.float32).ravel()
        check(np.ascontiguousarray(num), np.ascontiguousarray(den))
    # (b) extreme mantissas on every exponent pair
    mant = np.array([0, 1, 2, 0x400000, 0x3FFFFF, 0x7FFFFF, 0x7FFFFE, 0x555555, 0x2AAAAA], np.uint32)
    e1, e2, m1, m2 = np.meshgrid(exps, exps, mant, mant, indexing="ij")
    num = ((e1 << 23) | m1).astype(np.uint32).view(np.float32).ravel()
    den = ((e2 << 23) | m2).astype(np.uint32).view(np.float32).ravel()
    check(np.ascontiguousarray(num), np.ascontiguousarray(-den))
    # (c) specials: zeros, denormals, inf, NaN go through the plain division inside the hook
    sp = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, 3e38, np.inf, -np.inf, np.nan, 1.0, -3.0], np.float32)
    a, b = np.meshgrid(sp, sp, indexing="ij")
    check(np.ascontiguousarray(a.ravel()), np.ascontiguousarray(b.ravel()))


# ---- the drop-in class ---------------------------------------------------------------
class _M:  # any object with the three attributes is a model (duck typing)
    def __init__(self, tri, col, nrm):
        self._vertices_by_triangles, self._colors_by_triangles, self._normals_by_triangles = tri, col, nrm


def test_filler_drop_in_api(oracle):
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    filler = AdvancedPixelBufferFiller(200, 320, fov=45, n_threads=8, track_winner=True)
    assert filler.get_size() == (200, 320)
    assert filler.render_model(_M(tri, col, nrm)) is None
    f = oracle.OracleFiller(200, 320, fov=45)
    f.render_arrays(tri, col, nrm)
    z = filler.get_z_buffer()
    assert z.dtype == np.float32 and z.shape == (200, 320) and z.flags.writeable
    assert_bit_equal(z, f.z_buffer, "z")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
    assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "normal")
    assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "winner")
    assert filler.get_color_buffer() is filler.get_color_buffer()      # stable views
    # in-place edits of a getter's array are seen by the next render (guro_illumination.py:27)
    filler.get_color_buffer()[...] *= 0.5
    f.color_buffer *= 0.5
    cube = scene("cube_inputs.npz")
    filler.render_model(_M(*cube))
    f.render_arrays(*cube)
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z after 2nd model")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour after 2nd model")
    filler.clear()
    assert (filler.get_z_buffer() == 1e6).all() and (filler.get_color_buffer() == 0).all()


def test_filler_error_behaviour():
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("cube_inputs.npz")
    filler = AdvancedPixelBufferFiller(64, 64, fov=45)
    with pytest.raises(AttributeError):          # untextured model: colours are None
        filler.render_model(_M(tri, None, nrm))
    with pytest.raises(ValueError, match="double"):
        filler.render_model(_M(tri.astype(np.float64), col, nrm))
    with pytest.raises(ValueError):
        filler.render_model(_M(tri[:, :2], col, nrm))


def test_filler_recovers_from_bin_overflow(oracle):
    """General binning path with far too small a list capacity: the getter notices, grows the
    plan and renders the frame again."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(21)
    tri, col, nrm = random_soup(rng, 400, 512, size_px=(150, 400), frac_backface=0.0)
    filler = AdvancedPixelBufferFiller(512, 512, fov=45, tile=32, bin_capacity=500, direct_bins=False)
    filler.render_arrays(tri, col, nrm)
    need, cap = filler.bin_usage()
    assert cap == 500 and need > cap            # this frame dropped fragments ...
    f = oracle.OracleFiller(512, 512, fov=45)
    f.render_arrays(tri, col, nrm)
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z")   # ... the getter grows and redoes it
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
    need2, cap2 = filler.bin_usage()
    assert need2 == need and cap2 >= need


def test_filler_recovers_from_direct_bin_overflow(oracle):
    """Small-scene direct bins hold 1024 entries per tile; 3000 triangles stacked in one tile
    overflow them: the filler switches to the general path and the result is exact."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(22)
    tri, col, nrm = random_soup(rng, 5000, 256, size_px=(2, 6), frac_backface=0.0, margin=-0.97)
    filler = AdvancedPixelBufferFiller(256, 256, fov=45, tile=32)
    filler.render_arrays(tri, col, nrm)
    need, cap = filler.bin_usage()
    assert cap == 1024 and need > cap
    f = oracle.OracleFiller(256, 256, fov=45)
    f.render_arrays(tri, col, nrm)
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
    assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "normal")
    need2, cap2 = filler.bin_usage()
    assert need2 <= cap2 and cap2 != 1024       # general path now


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_pipelined_frames_are_exact(oracle, depth):
    """render_frame in pipeline mode is a swap chain: up to `depth` frames in flight on as many
    streams, plans and framebuffer sets.  Whatever the interleaving, the filler's buffers after
    frame N are frame N's: checked after bursts of frames and after switching the resident model
    mid-stream."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    trex = scene("trex_inputs.npz")
    cube = scene("cube_inputs.npz")
    rng = np.random.default_rng(4)
    soup = random_soup(rng, 20000, 300, size_px=(1, 30))
    H, W = 300, 420
    filler = AdvancedPixelBufferFiller(H, W, fov=45, pipeline=True, pipeline_depth=depth, track_winner=True)
    for model, bursts in ((trex, (1, 2, 7)), (soup, (3, 1)), (cube, (2,)), (trex, (5,))):
        f = oracle.OracleFiller(H, W, fov=45)
        f.render_arrays(*model)
        filler.render_arrays(*model, clear=True)       # upload; plain (non-pipelined) frame
        for burst in bursts:
            for _ in range(burst):
                filler.render_frame()
            assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z")
            assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
            assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "normal")
            assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "winner")
        filler.render_frame(pipelined=False)            # mixing plain frames in is fine too
        assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z after a plain frame")


def test_pipeline_c_abi_frame_bind_submit(oracle, hip):
    """crender_pipeline_* called directly: frames with explicit arguments and frames from bound
    slots give the oracle's buffers in every framebuffer set; an unbound slot is refused."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi
    L = hip
    lib = _capi.load()
    tri, col, nrm = scene("trex_inputs.npz")
    H, W, depth = 200, 260, 3
    f = oracle.OracleFiller(H, W, fov=45)
    f.render_arrays(tri, col, nrm)
    P = L.projection_matrix(45, 0.1, 1000.0, H, W)
    d = [torch.from_numpy(a).cuda() for a in (tri, col, nrm)]
    T = d[0].shape[0]
    plans = [L.Plan(H, W, T) for _ in range(depth)]
    fbs = [L.FrameBuffers(H, W, winner=True) for _ in range(depth)]
    arr = (C.c_void_p * depth)(*[p.handle.value for p in plans])
    pipe = C.c_void_p()
    _capi.check(lib.crender_pipeline_create(C.byref(pipe), arr, depth), "create")
    stream = torch.cuda.current_stream().cuda_stream
    try:
        assert lib.crender_pipeline_submit(pipe, stream) == _capi.EINVAL       # nothing bound yet
        for k, fb in enumerate(fbs):                                           # explicit arguments
            _capi.check(lib.crender_pipeline_frame(
                pipe, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), T, _capi.f32_16(P),
                fb.z.data_ptr(), fb.color.data_ptr(), fb.normals.data_ptr(), fb.winner.data_ptr(),
                _capi.FUSED_CLEAR, stream), "frame")
        _capi.check(lib.crender_pipeline_join(pipe, stream), "join")
        for fb in fbs:
            z, c, n, w = fb.numpy()
            assert_bit_equal(z, f.z_buffer, "z (frame)")
            assert_bit_equal(w, f.winner, "winner (frame)")
        assert lib.crender_pipeline_bind(pipe, depth, 0, 0, 0, 0, None, 0, 0, 0, 0, 0) == _capi.EINVAL
        for k, fb in enumerate(fbs):                                           # bound slots
            fb.z.fill_(-7.0)
            _capi.check(lib.crender_pipeline_bind(
                pipe, k, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), T, _capi.f32_16(P),
                fb.z.data_ptr(), fb.color.data_ptr(), fb.normals.data_ptr(), fb.winner.data_ptr(),
                _capi.FUSED_CLEAR), "bind")
        for _ in range(2 * depth + 1):
            _capi.check(lib.crender_pipeline_submit(pipe, stream), "submit")
        _capi.check(lib.crender_pipeline_join(pipe, stream), "join")
        for fb in fbs:
            z, c, n, w = fb.numpy()
            assert_bit_equal(z, f.z_buffer, "z (submit)")
            assert_bit_equal(c, f.color_buffer, "colour (submit)")
            assert_bit_equal(n, f.normals_buffer, "normal (submit)")
            assert_bit_equal(w, f.winner, "winner (submit)")
    finally:
        torch.cuda.synchronize()
        lib.crender_pipeline_destroy(pipe)


def test_lookahead_sees_inputs_rewritten_in_place(oracle):
    """Frames binned ahead survive a join only for inputs nobody else can write (the filler's own
    copies of numpy arrays: CRENDER_STATIC_INPUTS).  Device tensors handed in by the caller are used
    as they are, and when the caller rewrites them in place between bursts the next frames show the
    new contents."""
    import torch
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    moved = tri.copy()
    moved[:, :, 0] += np.float32(0.03)
    res = 512
    fa, fb = oracle.OracleFiller(res, res, fov=45), oracle.OracleFiller(res, res, fov=45)
    fa.render_arrays(tri, col, nrm)
    fb.render_arrays(moved, col, nrm)
    d = [torch.from_numpy(a).cuda() for a in (tri, col, nrm)]
    filler = AdvancedPixelBufferFiller(res, res, fov=45, pipeline=True, lookahead=True)
    filler.render_arrays(*d, clear=True)
    assert not filler._inputs_private
    for _ in range(6):
        filler.render_frame()
    assert_bit_equal(filler.get_z_buffer(), fa.z_buffer, "caller's tensors: z")
    d[0].copy_(torch.from_numpy(moved))                     # same addresses, new contents
    torch.cuda.synchronize()
    for _ in range(6):
        filler.render_frame()
    assert_bit_equal(filler.get_z_buffer(), fb.z_buffer, "rewritten in place: z")
    assert_bit_equal(filler.get_color_buffer(), fb.color_buffer, "rewritten in place: colour")
    own = AdvancedPixelBufferFiller(res, res, fov=45, pipeline=True, lookahead=True)
    own.render_arrays(tri, col, nrm, clear=True)            # numpy: the filler's own copies
    assert own._inputs_private
    for burst in (5, 1, 3):
        for _ in range(burst):
            own.render_frame()
        assert_bit_equal(own.get_z_buffer(), fa.z_buffer, f"own copies, burst of {burst}: z")
    own.render_arrays(moved, col, nrm, clear=True)          # new arrays of the same size (maybe at old addresses)
    for _ in range(5):
        own.render_frame()
    assert_bit_equal(own.get_z_buffer(), fb.z_buffer, "own copies replaced: z")
    assert_bit_equal(own.get_normals_buffer(), fb.normals_buffer, "own copies replaced: normal")


@pytest.mark.parametrize("H,W,flags_extra", [(1024, 1024, 0), (1024, 1024, 4), (700, 900, 0)])
def test_pipeline_c_abi_lookahead(oracle, hip, H, W, flags_extra):
    """crender_pipeline_set_lookahead called directly: argument errors; frames whose raster launch
    also bins the slot's next frame, as LONE frames (ordered dispatch, split heavy tiles: flags
    without CRENDER_OVERLAPPED_FRAMES) and as overlapped ones; another model in between, a frame
    of projected input (cannot look ahead) in between, a join in between; every framebuffer set
    ends up the oracle's frame of what it was last asked to render."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi
    L = hip
    lib = _capi.load()
    tri, col, nrm = scene("trex_inputs.npz")
    ctri, ccol, cnrm = scene("cube_inputs.npz")
    depth = 3
    ft, fc = oracle.OracleFiller(H, W, fov=45), oracle.OracleFiller(H, W, fov=45)
    ft.render_arrays(tri, col, nrm)
    fc.render_arrays(ctri, ccol, cnrm)
    P = L.projection_matrix(45, 0.1, 1000.0, H, W)
    d = [torch.from_numpy(a).cuda() for a in (tri, col, nrm)]
    dc = [torch.from_numpy(a).cuda() for a in (ctri, ccol, cnrm)]
    T, Tc = d[0].shape[0], dc[0].shape[0]
    plans = [L.Plan(H, W, T) for _ in range(2 * depth)]
    other = L.Plan(H, W, T + 5)
    fbs = [L.FrameBuffers(H, W, winner=True) for _ in range(depth)]
    arr = (C.c_void_p * depth)(*[p.handle.value for p in plans[:depth]])
    more = (C.c_void_p * depth)(*[p.handle.value for p in plans[depth:]])
    pipe = C.c_void_p()
    _capi.check(lib.crender_pipeline_create(C.byref(pipe), arr, depth), "create")
    stream = torch.cuda.current_stream().cuda_stream
    flags = _capi.FUSED_CLEAR | flags_extra

    def frame(inputs, n, k):
        fb = fbs[k]
        _capi.check(lib.crender_pipeline_frame(
            pipe, inputs[0].data_ptr(), inputs[1].data_ptr(), inputs[2].data_ptr(), n, _capi.f32_16(P),
            fb.z.data_ptr(), fb.color.data_ptr(), fb.normals.data_ptr(), fb.winner.data_ptr(), flags, stream), "frame")

    def check(expect, what):
        _capi.check(lib.crender_pipeline_join(pipe, stream), "join")
        for k, fb in enumerate(fbs):
            z, c, n, w = fb.numpy()
            f = expect[k]
            assert_bit_equal(z, f.z_buffer, f"{what}: set {k} z")
            assert_bit_equal(c, f.color_buffer, f"{what}: set {k} colour")
            assert_bit_equal(n, f.normals_buffer, f"{what}: set {k} normal")
            assert_bit_equal(w, f.winner, f"{what}: set {k} winner")

    try:
        assert lib.crender_pipeline_set_lookahead(pipe, more, depth - 1) == _capi.EINVAL          # one per slot
        assert lib.crender_pipeline_set_lookahead(pipe, arr, depth) == _capi.EINVAL               # not distinct
        bad = (C.c_void_p * depth)(*([p.handle.value for p in plans[depth:2 * depth - 1]] + [other.handle.value]))
        assert lib.crender_pipeline_set_lookahead(pipe, bad, depth) == _capi.EINVAL               # unlike plans
        _capi.check(lib.crender_pipeline_set_lookahead(pipe, more, depth), "set_lookahead")
        n = 0
        for burst in (1, 2, 3, 7):                         # T-Rex, bursts with joins in between
            for _ in range(burst):
                frame(d, T, n % depth); n += 1
            if n >= depth:
                check([ft] * depth, f"T-Rex after a burst of {burst}")
                n = 0
        for _ in range(depth):                             # every slot binned ahead for T-Rex: now the cube
            frame(d, T, n % depth); n += 1
        for _ in range(depth + 1):
            frame(dc, Tc, n % depth); n += 1
        check([fc] * depth, "cube after T-Rex without a join"); n = 0
        for i in range(2 * depth):                         # alternating models: nothing binned ahead ever fits
            frame(d if i % 2 == 0 else dc, T if i % 2 == 0 else Tc, n % depth); n += 1
        last = {}
        for i in range(2 * depth):
            last[i % depth] = ft if i % 2 == 0 else fc
        check([last[k] for k in range(depth)], "alternating models"); n = 0
        assert lib.crender_pipeline_set_lookahead(pipe, None, 0) == _capi.OK                      # off again
        for _ in range(depth + 2):
            frame(d, T, n % depth); n += 1
        check([ft] * depth, "look-ahead switched off")
    finally:
        torch.cuda.synchronize()
        lib.crender_pipeline_destroy(pipe)


@pytest.mark.parametrize("res,tile,clear,depth,overlapped", [
    (512, 32, True, 1, 0), (512, 32, False, 1, 0), (1024, 32, True, 1, 0), (512, 16, True, 1, 0),
    (512, 32, True, 2, 0), (512, 32, True, 3, 4), (640, 0, False, 3, 4), (512, 32, False, 2, 0), (384, 16, True, 4, 4)])
def test_lone_chain_through_changing_scenes(oracle, hip, res, tile, clear, depth, overlapped):
    """The swap chain with look-ahead fed a DIFFERENT scene every few frames.  depth 1 is the chain bench.py's
    `roofline` view dispatches: one frame at a time, k_frame, every covered 32-pixel tile in four quadrants
    through flag and helper-slot words, dispatch in the previous frame's order, the slot's NEXT frame binned
    ahead into its other plan.  Deeper chains rotate framebuffer sets and plans; with CRENDER_OVERLAPPED_FRAMES
    (4) the frames are not split.  Scenes: T-Rex (small records), the cube (a few large triangles: the pixel
    owners' tiles), a soup that touches more tiles than the plans have helper triples, a few large triangles,
    no triangles.  Whatever the previous launches left behind — an order for other tiles, hand-off words,
    bins filled ahead for another model — every framebuffer set is the oracle's, bit for bit."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi
    L, lib = hip, _capi.load()
    H = W = res
    trex = scene("trex_inputs.npz")
    cube = scene("cube_inputs.npz")
    big = random_soup(np.random.default_rng(11), 4000, H, size_px=(2, 14))
    few = random_soup(np.random.default_rng(12), 60, H, size_px=(20, 90))
    none = tuple(np.zeros((0, 3, 3), np.float32) for _ in range(3))
    scenes_ = {"trex": trex, "cube": cube, "big": big, "few": few, "none": none}
    dev = {k: [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in v] for k, v in scenes_.items()}
    maxT = max(len(v[0]) for v in scenes_.values())
    P = L.projection_matrix(45, 0.1, 1000.0, H, W)
    plans = [L.Plan(H, W, maxT, tile=tile) for _ in range(2 * depth)]
    fbs = [L.FrameBuffers(H, W, winner=True) for _ in range(depth)]
    pipe = C.c_void_p()
    first = (C.c_void_p * depth)(*[p.handle.value for p in plans[:depth]])
    second = (C.c_void_p * depth)(*[p.handle.value for p in plans[depth:]])
    _capi.check(lib.crender_pipeline_create(C.byref(pipe), first, depth), "create")
    stream = torch.cuda.current_stream().cuda_stream
    flags = (_capi.FUSED_CLEAR if clear else 0) | overlapped
    refs = [oracle.OracleFiller(H, W, fov=45.0) for _ in range(depth)]
    order = ["trex", "trex", "trex", "cube", "cube", "trex", "big", "big", "cube", "none", "trex", "few", "few",
             "big", "none", "none", "cube", "trex", "few", "cube", "big", "trex", "trex", "cube", "few", "trex"]
    try:
        _capi.check(lib.crender_pipeline_set_lookahead(pipe, second, depth), "set_lookahead")
        for k, name in enumerate(order):
            t, c, n = dev[name]
            slot = k % depth
            ref, fb = refs[slot], fbs[slot]
            if clear:
                ref.clear()
            ref.render_arrays(*scenes_[name])
            _capi.check(lib.crender_pipeline_frame(
                pipe, t.data_ptr(), c.data_ptr(), n.data_ptr(), t.shape[0], _capi.f32_16(P),
                fb.z.data_ptr(), fb.color.data_ptr(), fb.normals.data_ptr(), fb.winner.data_ptr(), flags, stream),
                "frame")
            if k % 3 != 1:            # (frames in a row without a join now and then)
                _capi.check(lib.crender_pipeline_join(pipe, stream), "join")
                torch.cuda.synchronize()
                for q_, plan in enumerate(plans):     # rasterized plans and plans binned ahead alike: their state first
                    try:
                        plan.debug_check()
                    except Exception as e:
                        raise AssertionError(f"frame {k} ({name} after {order[k - 1] if k else '-'}), plan {q_}, {res}^2, "
                                             f"tile {tile}, clear={clear}, depth {depth}, flags {flags}: {e}") from e
                for s_, (r_, b_) in enumerate(zip(refs, fbs)):
                    z, cc, nn, w = b_.numpy()
                    what = (f"frame {k} ({name} after {order[k - 1] if k else '-'}), set {s_}, {res}^2, tile {tile}, "
                            f"clear={clear}, depth {depth}, flags {flags}")
                    assert_bit_equal(z, r_.z_buffer, what + ": z")
                    assert_bit_equal(cc, r_.color_buffer, what + ": colour")
                    assert_bit_equal(nn, r_.normals_buffer, what + ": normal")
                    if clear:
                        assert_bit_equal(w, r_.winner, what + ": winner")
    finally:
        torch.cuda.synchronize()
        lib.crender_pipeline_destroy(pipe)


@pytest.mark.parametrize("direction", [[0.3, -0.2, 1], [0, 0, 1]])
def test_renderer_with_illumination(oracle, direction):
    """Renderer.render in its four forms against the oracle's render + the oracle's own C
    restatement of guro_illumination.py:20-27 (``oracle.guro``, pinned against numpy's evaluation of
    the reference's statements on the CPU).  Light [0, 0, 1] is the signed-zero case: every product
    of a background pixel's zero normal with the flipped light is -0 and numpy's reduction, which
    starts from +0, yields +0."""
    from cython3dmodelrenderer_amd import Renderer
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    light = GuroIllumination(direction)
    f = oracle.OracleFiller(256, 256, fov=45)
    f.render_arrays(tri, col, nrm)
    oracle.guro(f.color_buffer, f.normals_buffer, direction)
    host = Renderer(AdvancedPixelBufferFiller(256, 256, fov=45), light, None, 256, 256, on_device=False)
    img = host.render(_M(tri, col, nrm))
    assert_bit_equal(img, f.color_buffer, "Renderer.render (numpy illumination)")
    # the default: shading on the device, the reference's return value (the writable numpy view)
    auto_filler = AdvancedPixelBufferFiller(256, 256, fov=45)
    auto = Renderer(auto_filler, light, None, 256, 256)
    img_a = auto.render(_M(tri, col, nrm))
    assert isinstance(img_a, np.ndarray) and img_a.flags.writeable
    assert_bit_equal(img_a, f.color_buffer, "Renderer.render (default: HIP illumination, numpy view)")
    assert "normals" not in auto_filler._host          # only the colour plane crossed PCIe
    # a second render composites on the shaded buffer, as in the reference (reset_buffers is a no-op)
    cube = scene("cube_inputs.npz")
    f.render_arrays(*cube)
    oracle.guro(f.color_buffer, f.normals_buffer, direction)
    img_b = auto.render(_M(*cube))
    assert img_b is img_a
    assert_bit_equal(img_b, f.color_buffer, "Renderer.render twice (composite on the shaded buffer)")
    f = oracle.OracleFiller(256, 256, fov=45)
    f.render_arrays(tri, col, nrm)
    oracle.guro(f.color_buffer, f.normals_buffer, direction)
    dev = Renderer(AdvancedPixelBufferFiller(256, 256, fov=45), light, None, 256, 256, on_device=True)
    img_d = dev.render(_M(tri, col, nrm)).cpu().numpy()
    assert_bit_equal(img_d, f.color_buffer, "Renderer.render (HIP illumination)")
    fused = Renderer(AdvancedPixelBufferFiller(256, 256, fov=45), light, None, 256, 256, on_device="fused")
    img_f = fused.render(_M(tri, col, nrm)).cpu().numpy()
    assert_bit_equal(img_f, f.color_buffer, "Renderer.render (illumination fused into the raster kernel)")


@pytest.mark.parametrize("seed", range(12 * _SOAK))
def test_fuzz_renderers_sharing_one_filler(oracle, seed):
    """Seeded sessions of ``Renderer.render`` (cy/renderer.py:47-49: render_model, draw_illumination on the
    WHOLE colour buffer, return it) through all four forms of this package's Renderer — numpy illumination on
    the host views, the default (shading on the device, the numpy view returned), on_device=True (the tensor)
    and "fused" (a frame from cleared buffers, shaded as it is stored) — taking turns on ONE filler, with bursts
    of render_frame and a clear() in between: renders composite on buffers that earlier renders have already
    shaded (the reference's behaviour: reset_buffers is a no-op), so every form must leave exactly the bits
    the next one starts from.  The oracle: its filler + its own C restatement of guro_illumination.py:20-27."""
    import torch
    from cython3dmodelrenderer_amd import Renderer
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(11000 + seed)
    H = int(rng.choice([192, 256, 320])); W = int(rng.choice([256, 384]))
    direction = [[0.3, -0.2, 1], [0, 0, 1], [-0.5, 0.4, 0.7]][seed % 3]
    light = GuroIllumination(direction)
    kw = {"pipeline": True} if seed % 2 else {}
    filler = AdvancedPixelBufferFiller(H, W, fov=45, **kw)
    forms = {m: Renderer(filler, light, None, H, W, on_device=m) for m in (False, None, True, "fused")}
    ref = oracle.OracleFiller(H, W, fov=45.0)
    pool = {"trex": scene("trex_inputs.npz"), "cube": scene("cube_inputs.npz"),
            "small": random_soup(rng, 1500, max(H, W), size_px=(1, 9)),
            "large": random_soup(rng, 40, max(H, W), size_px=(20, 110))}
    names = list(pool)
    story = []
    for step in range(18):
        name = names[int(rng.integers(0, len(names)))]
        form = [False, None, None, True, "fused", "frames", "clear"][int(rng.integers(0, 7))]
        story.append((form, name))
        if form == "clear":
            filler.clear(); ref.clear()
            continue
        if form == "frames":
            # (the swap chain's frames shade too once an illumination has been fused into the filler)
            if filler._inputs is None:
                continue
            last = story_last_inputs
            for _ in range(int(rng.integers(1, 4))):
                filler.render_frame()
            ref.clear()
            ref.render_arrays(*last)
            if filler._fused_light is not None:
                oracle.guro(ref.color_buffer, ref.normals_buffer, direction)
            got = filler.get_color_buffer()
        else:
            if form == "fused":
                ref.clear()
            ref.render_arrays(*pool[name])
            oracle.guro(ref.color_buffer, ref.normals_buffer, direction)
            img = forms[form].render(_M(*pool[name]))
            got = img.cpu().numpy() if isinstance(img, torch.Tensor) else img
            story_last_inputs = pool[name]
        what = f"renderer session {seed} ({H}x{W}, {kw}, light {direction}), step {step} of {story}"
        if got is not None and isinstance(got, np.ndarray):
            got = got.copy()            # (the check below settles the filler: keep what this step returned)

        def state():                    # the plans' cross-frame state (crender_plan_debug_check); it synchronises
            try:
                filler.debug_check()
            except Exception as e:
                raise AssertionError(f"{what}: {e}") from e
        if step % 2 == 0:
            state()                     # even steps: before the pixels; odd ones: the getters meet the frames in flight
        assert_bit_equal(got, ref.color_buffer, what + ": colour")
        assert_bit_equal(filler.get_z_buffer(), ref.z_buffer, what + ": z")
        assert_bit_equal(filler.get_normals_buffer(), ref.normals_buffer, what + ": normal")
        if step % 2:
            state()


@pytest.mark.parametrize("res,tile", [(256, 0), (300, 32), (192, 64), (1024, 0)])
def test_fused_guro_equals_the_separate_pass(oracle, hip, res, tile):
    """CRENDER_FUSED_GURO: the raster kernel shades each pixel as it stores it.  Bit for bit the
    numpy form on the oracle's buffers (= the reference's draw_illumination after render_model on
    fresh buffers) and the separate HIP pass, on every tile size, through the plain and the
    pipelined frame path; normals and z are untouched; a compositing frame refuses the flag."""
    from cython3dmodelrenderer_amd import Renderer, _capi
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    light = GuroIllumination([0.3, -0.2, 1])
    f = oracle.OracleFiller(res, res, fov=45)
    f.render_arrays(tri, col, nrm)
    oracle.guro(f.color_buffer, f.normals_buffer, [0.3, -0.2, 1])
    filler = AdvancedPixelBufferFiller(res, res, fov=45, tile=tile, pipeline=True)
    fused = Renderer(filler, light, None, res, res, on_device="fused")
    img = fused.render(_M(tri, col, nrm)).cpu().numpy()
    assert_bit_equal(img, f.color_buffer, "fused illumination: colour")
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "fused illumination: z")
    assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "fused illumination: normal")
    for _ in range(5):                       # swap-chain frames carry the light too
        filler.render_frame()
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "fused illumination, pipelined frames")
    filler.set_fused_illumination(None)
    filler.render_frame(pipelined=False)
    unlit = oracle.OracleFiller(res, res, fov=45)
    unlit.render_arrays(tri, col, nrm)
    assert_bit_equal(filler.get_color_buffer(), unlit.color_buffer, "fusion switched off again")
    # the C ABI refuses the flag on a frame that composites
    P = hip.projection_matrix(45.0, 0.1, 1000.0, res, res)
    plan = hip.Plan(res, res, len(tri), tile=tile)
    fb = hip.FrameBuffers(res, res)
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    lib = _capi.load()
    rc = lib.crender_render_model(plan.handle, t.data_ptr(), c.data_ptr(), n.data_ptr(), len(tri),
                                  _capi.f32_16(P), fb.z.data_ptr(), fb.color.data_ptr(),
                                  fb.normals.data_ptr(), None, _capi.FUSED_GURO, None)
    assert rc == _capi.EINVAL and b"FUSED_CLEAR" in lib.crender_last_error()


def test_present_u8_matches_numpy_cast(oracle):
    """Row f3: image[::-1].astype('uint8') (reference: run.py:26) on the device, and the whole
    run.py pipeline against the reference's committed render."""
    from PIL import Image
    from cython3dmodelrenderer_amd import Renderer
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    filler = AdvancedPixelBufferFiller(1024, 1024, fov=45)
    r = Renderer(filler, GuroIllumination([0, 0, 1]), None, 1024, 1024, on_device=True)
    img = r.render(_M(tri, col, nrm)).cpu().numpy()
    got = filler.present_u8().cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (1024, 1024, 3)
    assert (got == img[::-1].astype("uint8")).all()
    ref_rgb = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "reference_output_T-Rex.png")).convert("RGB"))
    assert (got[:, :, ::-1] != ref_rgb).any(axis=-1).sum() <= 200     # ~116 racy pixels
    # cast semantics on awkward values
    import torch
    vals = np.array([0.0, 0.99, 1.0, 254.999, 255.0, 255.5, 256.0, 300.7, -0.5, -1.0, -1.5, 1e9, -1e9],
                    np.float32)
    plane = np.resize(vals, (2, 8, 3)).astype(np.float32)
    f2 = AdvancedPixelBufferFiller(2, 8, fov=45)
    f2.color_buffer.copy_(torch.from_numpy(plane))
    with np.errstate(invalid="ignore"):
        want = plane[::-1].astype("uint8")
    got2 = f2.present_u8().cpu().numpy()
    inrange = (plane[::-1] > -2**31) & (plane[::-1] < 2**31)
    assert (got2[inrange] == want[inrange]).all()


# ---- full BASELINE.json sizes ----------------------------------------------------------
@pytest.mark.parametrize("name,fixture,res", [("bunny4096", "bunny_inputs.npz", 4096),
                                              ("trex8192", "trex_inputs.npz", 8192)])
def test_full_size_configs_match_golden(hip, golden, name, fixture, res):
    """configs[2] and configs[3] at full resolution against the oracle's hashes (the oracle's
    work counts at these sizes were checked against the reference run)."""
    tri, col, nrm = scene(fixture)
    g = golden["scenes"][name]
    got = gpu_frame(hip, tri, col, nrm, res, res, mode="fused", clear=True)
    assert int((got[0] < 1e6).sum()) == g["covered"]
    assert (sha(got[0]), sha(got[1]), sha(got[2]), sha(got[3])) == (g["z"], g["c"], g["n"], g["winner"])
    again = gpu_frame(hip, tri, col, nrm, res, res, mode="atomic")
    for a, b, what in zip(got[:4], again[:4], ("z", "colour", "normal", "winner")):
        assert_bit_equal(a, b, f"{name}: tile path vs atomic path, {what}")


def test_trex8192_eight_row_strips(hip, golden):
    """configs[3] as the 8 strips of 1024 rows the multi-GPU layout uses."""
    tri, col, nrm = scene("trex_inputs.npz")
    strips = [(i * 1024, (i + 1) * 1024) for i in range(8)]
    got = gpu_frame(hip, tri, col, nrm, 8192, 8192, mode="fused", strips=strips, clear=True)
    g = golden["scenes"]["trex8192"]
    assert (sha(got[0]), sha(got[1]), sha(got[2])) == (g["z"], g["c"], g["n"])


def test_synthetic_small_triangles_at_4096(hip, oracle):
    """configs[4] recipe at 2M triangles (the 10M run lives in bench.py): tile path vs oracle
    vs atomic path, plus idempotence (drawing the same triangles again changes nothing)."""
    from cython3dmodelrenderer_amd import scenes
    tri, col, nrm = scenes.synthetic_triangles(2_000_000, res=4096)
    f = oracle_frame(oracle, tri, col, nrm, 4096, 4096)
    got = gpu_frame(hip, tri, col, nrm, 4096, 4096, mode="fused", clear=True)
    compare(got, f, "synthetic 2M")
    at = gpu_frame(hip, tri, col, nrm, 4096, 4096, mode="atomic")
    compare(at, f, "synthetic 2M atomic")
    twice = gpu_frame(hip, tri, col, nrm, 4096, 4096, mode="fused", prior=got[:3])
    for a, b, what in zip(got[:3], twice[:3], ("z", "colour", "normal")):
        assert_bit_equal(a, b, f"idempotence: {what}")


@pytest.mark.parametrize("tile", [16, 32])
@pytest.mark.parametrize("clear", [True, False])
def test_dispatch_order_hint_never_changes_pixels(hip, oracle, clear, tile):
    """On small frames each raster launch leaves a dispatch order for the next launch on the same
    plan (covered tiles first, empty tiles cleared in groups without a look at their lists).  The
    order is a hint about speed only: frames of the same model, of another model (stale order), of
    the model moved by a few pixels and by half a frame, and of no triangles at all, rendered one
    after another on ONE plan, must each equal the oracle bit for bit.  On 32-pixel tiles every covered
    tile is split among four workgroups through a table of helper slots, and an ordered launch counts the
    slots in use and sends the rest to the end of its grid: the soup covers more tiles than there are
    slots, the cube and T-Rex fewer, the empty frame none — in every order of succession."""
    H = W = 512
    tri, col, nrm = scene("trex_inputs.npz")
    ctri, ccol, cnrm = scene("cube_inputs.npz")
    rng = np.random.default_rng(5)
    stri, scol, snrm = random_soup(rng, 400, H, size_px=(2, 30))

    def moved(dx, dy):
        t = tri.copy()
        t[..., 0] += np.float32(dx) * t[..., 2]
        t[..., 1] += np.float32(dy) * t[..., 2]
        return t

    e = np.zeros((0, 3, 3), np.float32)
    frames = [(tri, col, nrm), (tri, col, nrm), (tri, col, nrm), (moved(0.01, 0.0), col, nrm),
              (moved(0.02, 0.01), col, nrm), (ctri, ccol, cnrm), (ctri, ccol, cnrm), (tri, col, nrm),
              (e, e, e), (tri, col, nrm), (moved(0.4, -0.3), col, nrm), (stri, scol, snrm),
              (stri, scol, snrm), (tri, col, nrm)]
    P = hip.projection_matrix(45.0, 0.1, 1000.0, H, W)
    plan = hip.Plan(H, W, max(len(tri), len(stri)), tile=tile)
    fb = hip.FrameBuffers(H, W)
    ref = oracle.OracleFiller(H, W, fov=45.0)
    if tile == 32:
        # (a soup that touches more tiles than the plan has helper triples — 256 tiles, 128 triples)
        s2 = random_soup(np.random.default_rng(6), 3000, H, size_px=(2, 12))
        frames = frames + [s2, (tri, col, nrm), s2, s2, (e, e, e), s2, (ctri, ccol, cnrm)]
        plan = hip.Plan(H, W, max(len(tri), len(stri), len(s2[0])), tile=tile)
    for k, (t, c, n) in enumerate(frames):
        if clear:
            ref.clear()
        ref.render_arrays(t, c, n)
        if len(t):
            hip.render_model(plan, _dev(t), _dev(c), _dev(n), P, fb, clear=clear)
        else:
            import torch
            z = torch.zeros((0, 3, 3), dtype=torch.float32, device="cuda:0")
            hip.render_model(plan, z, z, z, P, fb, clear=clear)
        need, cap = plan.bin_usage()
        assert need <= cap and plan.last_frame_direct()
        try:
            plan.debug_check()          # the state this frame leaves (crender_plan_debug_check), before any pixel shows it
        except Exception as e_:
            raise AssertionError(f"frame {k} on one plan (clear={clear}, tile={tile}): {e_}") from e_
        compare(tuple(fb.numpy()) + (None,), ref, f"frame {k} on one plan (clear={clear}, tile={tile})")


def test_synthetic_10m_matches_golden(hip, golden):
    """configs[4] at FULL size: 10 M synthetic triangles at 4096 x 4096 through the tile path
    against the oracle's hashes (tests/golden/golden.json, made by scripts/make_golden.py in the
    build container) and, plane by plane, against the independent atomic path."""
    from cython3dmodelrenderer_amd import scenes
    tri, col, nrm = scenes.synthetic_triangles(10_000_000, res=4096)
    g = golden["scenes"]["synth10m"]
    got = gpu_frame(hip, tri, col, nrm, 4096, 4096, mode="fused", clear=True)
    assert int((got[0] < 1e6).sum()) == g["covered"]
    assert (sha(got[0]), sha(got[1]), sha(got[2]), sha(got[3])) == (g["z"], g["c"], g["n"], g["winner"])
    again = gpu_frame(hip, tri, col, nrm, 4096, 4096, mode="atomic")
    for a, b, what in zip(got[:4], again[:4], ("z", "colour", "normal", "winner")):
        assert_bit_equal(a, b, f"synth10m: tile path vs atomic path, {what}")


@pytest.mark.parametrize("res,tile,depth", [(512, 0, 0), (1024, 0, 0), (1536, 0, 0), (512, 0, 1), (1024, 0, 1)])
def test_pipeline_lookahead_bins_the_next_frame_in_the_raster_launch(oracle, res, tile, depth):
    """Swap chain with look-ahead (crender_pipeline_set_lookahead): every launch rasterizes one frame
    and bins the slot's next one into a second plan.  Frames must be the oracle's whatever the
    history: bursts of any length, a join in between, another model (the plans were binned ahead for
    the old one), back again, and look-ahead off for comparison — 16- and 32-pixel tiles.  depth 1: the
    chain renders every frame ALONE — covered 32-pixel tiles in four quadrants through the helper slots,
    dispatch in the previous frame's order — and the cube's tiles (a few large triangles each: the pixel
    owners') give way to T-Rex's (small records) and back."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    ctri, ccol, cnrm = scene("cube_inputs.npz")
    ft, fc = oracle.OracleFiller(res, res, fov=45), oracle.OracleFiller(res, res, fov=45)
    ft.render_arrays(tri, col, nrm)
    fc.render_arrays(ctri, ccol, cnrm)

    def check(filler, f, what):
        assert_bit_equal(filler.get_z_buffer(), f.z_buffer, f"{what}: z")
        assert_bit_equal(filler.get_color_buffer(), f.color_buffer, f"{what}: colour")
        assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, f"{what}: normal")
        assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, f"{what}: winner")

    for look in (True, False):
        filler = AdvancedPixelBufferFiller(res, res, fov=45, tile=tile, pipeline=True, track_winner=True,
                                           lookahead=look, **({"pipeline_depth": depth} if depth else {}))
        filler.render_arrays(tri, col, nrm, clear=True)
        assert filler._pipe is None or filler._pipe.lookahead == look
        for burst in (1, 2, 3, 4, 5, 9):
            for _ in range(burst):
                filler.render_frame()
            assert filler._pipe.lookahead == look
            check(filler, ft, f"look-ahead {look}, T-Rex after a burst of {burst}")
        filler.render_arrays(ctri, ccol, cnrm, clear=True)          # other inputs: nothing binned ahead fits
        for burst in (1, 6):
            for _ in range(burst):
                filler.render_frame()
            check(filler, fc, f"look-ahead {look}, cube after a burst of {burst}")
        none = np.zeros((0, 3, 3), np.float32)                      # frames of no triangles in between
        filler.render_arrays(none, none, none, clear=True)
        for _ in range(5):
            filler.render_frame()
        assert int((filler.get_z_buffer() != np.float32(1e6)).sum()) == 0, f"look-ahead {look}: empty frame"
        filler.render_arrays(tri, col, nrm, clear=True)
        for _ in range(7):
            filler.render_frame()
        check(filler, ft, f"look-ahead {look}, T-Rex again")
        for who, (a, b, c_), f in (("cube", (ctri, ccol, cnrm), fc), ("T-Rex", (tri, col, nrm), ft),
                                   ("cube", (ctri, ccol, cnrm), fc), ("T-Rex", (tri, col, nrm), ft)):
            filler.render_arrays(a, b, c_, clear=True)               # straight from one model to the other
            for _ in range(3):
                filler.render_frame()
            check(filler, f, f"look-ahead {look}, depth {depth}: {who} right after the other model")
        # every framebuffer set of the chain holds the frame
        for k, (z, c, n, w) in enumerate(filler._pipe.sets):
            assert_bit_equal(z.cpu().numpy(), ft.z_buffer, f"set {k}: z")
            assert_bit_equal(c.cpu().numpy(), ft.color_buffer, f"set {k}: colour")


@pytest.mark.parametrize("name,fixture,res,depth", [("bunny4096", "bunny_inputs.npz", 4096, 3),
                                                    ("trex8192", "trex_inputs.npz", 8192, 3)])
def test_pipelined_frames_at_bench_sizes(golden, name, fixture, res, depth):
    """The swap chain at the sizes bench.py pipelines: after bursts of frames in flight the
    filler's buffers are the golden frame, in every framebuffer set of the chain."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene(fixture)
    g = golden["scenes"][name]
    filler = AdvancedPixelBufferFiller(res, res, fov=45, pipeline=True, pipeline_depth=depth)
    filler.render_arrays(tri, col, nrm, clear=True)
    for burst in (1, depth, 2 * depth + 1):
        for _ in range(burst):
            filler.render_frame()
        assert (sha(filler.get_z_tensor().cpu().numpy()), sha(filler.get_color_tensor().cpu().numpy()),
                sha(filler.get_normals_tensor().cpu().numpy())) == (g["z"], g["c"], g["n"]), (name, burst)


_STRIP_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from cython3dmodelrenderer_amd import distributed as D
from cython3dmodelrenderer_amd import scenes
from oracle import oracle as O
rank = int(sys.argv[1])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=rank, world_size=2)
tri, col, nrm = scenes.load_fixture("trex_inputs.npz")
# (384 rows: equal strips; 383 rows: a ragged last strip and, with 3 sub-strips, ragged sub-strips)
for H, W, cases in ((384, 512, [(e, c, "local") for e in ("planes", "color", "present") for c in (1, 3)] + [("planes", 1, "broadcast")]),
                    (383, 320, [("planes", 3, "local"), ("present", 3, "local"), ("color", 2, "broadcast")])):
    full = O.OracleFiller(H, W, fov=45)
    full.render_arrays(tri, col, nrm)
    want_img = full.color_buffer[::-1].astype("uint8")
    for exchange, chunks, project in cases:
        # the PRODUCT's strip path (filler restricted to this rank's rows, HIP kernels) through a
        # collective; two ranks share the one GPU, gloo carries the strips through the host.
        # project="broadcast": rank 0 runs K1, the projected vertices are broadcast, both rasterize them
        sr = D.StripRenderer(H, W, rank, 2, fov=45, device="cuda:0", exchange=exchange, chunks=chunks, project=project)
        sr.set_model_arrays(tri, col, nrm)
        for _ in range(2):
            out = sr.render_frame()
        torch.cuda.synchronize()
        if exchange == "present":
            assert np.array_equal(out[0].cpu().numpy(), want_img), (H, exchange, chunks, project)
        else:
            wants = (full.z_buffer, full.color_buffer, full.normals_buffer) if exchange == "planes" else (full.color_buffer,)
            for got, want in zip(out, wants):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (H, exchange, chunks, project)
# ---- a SESSION per strip renderer: the model changes every few frames (T-Rex, the cube's few large triangles,
# a soup, no triangles), bursts of frames in between — every rank's plans, swap chain and exchange buffers carry
# state from one model's frames into the next one's
rng = np.random.default_rng(5)      # (the same soup on both ranks)
def soup(n, lo, hi, res):
    f = 2.4142137
    cz = rng.uniform(0.5, 3.0, (n, 1)).astype(np.float32)
    cxy = rng.uniform(-1.2 / f, 1.2 / f, (n, 2)).astype(np.float32) * cz
    centre = np.concatenate([cxy, cz], 1)[:, None, :]
    r = rng.uniform(lo, hi, (n, 1, 1)).astype(np.float32) * (2.0 / res) / f * cz[:, None, :]
    t = (centre + rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32) * r).astype(np.float32)
    nn = rng.standard_normal((n, 3, 3)).astype(np.float32); nn[..., 2] = -np.abs(nn[..., 2])
    return t, rng.uniform(0, 255, (n, 3, 3)).astype(np.float32), nn
cube = scenes.load_fixture("cube_inputs.npz")
H, W = 320, 384
pool = dict(trex=(tri, col, nrm), cube=cube, soup=soup(2500, 1, 12, W), few=soup(40, 20, 100, W))
for exchange, chunks, project in (("planes", 1, "local"), ("planes", 3, "local"), ("color", 2, "broadcast"), ("present", 1, "local")):
    sr = D.StripRenderer(H, W, rank, 2, fov=45, device="cuda:0", exchange=exchange, chunks=chunks, project=project)
    for step, name in enumerate(["trex", "cube", "trex", "soup", "few", "cube", "soup", "trex", "few", "trex"]):
        t, c, n = pool[name]
        full = O.OracleFiller(H, W, fov=45)
        full.render_arrays(t, c, n)
        sr.set_model_arrays(t, c, n)
        for _ in range(1 + step % 3):
            out = sr.render_frame()
        torch.cuda.synchronize()
        what = ("session", exchange, chunks, project, step, name)
        if exchange == "present":
            assert np.array_equal(out[0].cpu().numpy(), full.color_buffer[::-1].astype("uint8")), what
        else:
            wants = (full.z_buffer, full.color_buffer, full.normals_buffer) if exchange == "planes" else (full.color_buffer,)
            for got, want in zip(out, wants):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), what
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_two_ranks_strip_renderer_on_one_gpu(tmp_path):
    """north_star's sharded layout with the product's own strip path: two ranks (sharing the one
    GPU of the box) each rasterize their row strip with the HIP filler and exchange strips — all
    three planes, colour only, or the presented uint8 image, whole strips or sub-strips gathered
    on a second stream — and every rank ends up with the oracle's full frame."""
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "strip_worker.py"
    script.write_text(_STRIP_WORKER.format(root=ROOT, port=port))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, out
        assert f"rank {r} ok" in out


def test_device_model_transforms_match_host_model(oracle):
    """Row f2: shift / scale / mean vertex / max span / the *_by_triangles gathers on the device
    against the host Model (numpy, the reference's own call sequence) — bit for bit, through the
    README's fit (shift by a float32 array, scale by 1 / span, shift by a Python list: numpy
    promotes that sum to float64), a host-side rotate in between, and a render of the result."""
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.scenes import fit_model
    rng = np.random.default_rng(11)
    V, T = 1500, 2600
    vertices = (rng.standard_normal((V, 3)) * [3.0, 1.0, 0.5] + [10.0, -4.0, 2.0]).astype(np.float32)
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    host = Model(vertices, faces)
    host.set_uniform_color()
    dev = DeviceModel(Model(vertices, faces))
    dev.set_uniform_color()

    def same(what):
        assert_bit_equal(dev.get_mean_vertex(), host.get_mean_vertex(), f"{what}: mean vertex")
        assert np.float32(dev.get_max_span()).view(np.uint32) == np.float32(host.get_max_span()).view(np.uint32), what
        assert_bit_equal(dev._vertices.cpu().numpy(), host._vertices, f"{what}: vertices")
        assert_bit_equal(dev._vertices_by_triangles.cpu().numpy(), host._vertices_by_triangles, f"{what}: by triangles")
        assert_bit_equal(dev._normals_by_triangles.cpu().numpy(), host._normals_by_triangles, f"{what}: normals")

    same("upload")
    host.rotate([10, -80, 0])
    dev.rotate([10, -80, 0], on_host=True)
    same("rotate (host)")
    for m in (host, dev):
        fit_model(m)
    same("fit_model")
    for m in (host, dev):
        m.shift(np.array([0.25, -0.125, 3.0]))          # float64 array
        m.scale(0.37, keep_position=False)
        m.shift(np.float32(0.5) * np.ones(3, np.float32))
    same("more transforms")
    for m in (host, dev):
        fit_model(m)
    same("fit again")
    # and the filler takes the device arrays as they are
    f = oracle.OracleFiller(200, 200, fov=45)
    f.render_model(host)
    filler = AdvancedPixelBufferFiller(200, 200, fov=45)
    filler.render_model(dev)
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "render of the device model: z")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "render of the device model: colour")


def test_device_model_texture_colors_match_host_model():
    """Row f4's device part: the per-texture-coordinate colour lookup (reference model.py:143-151:
    nearest texel, v flipped, numpy's float32 arithmetic and truncating int32 cast) and the
    colours-by-triangles gather on the device against the host Model, bit for bit — texture
    coordinates inside, on the edges, outside [0, 1], huge, infinite and NaN, two and three columns,
    and faces that use an .obj file's negative (relative) indices."""
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    rng = np.random.default_rng(23)
    V, T, N = 400, 700, 900
    vertices = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(-V, V, (T, 3)).astype(np.int32)
    for cols, (th, tw) in ((2, (37, 53)), (3, (128, 64)), (2, (1, 1))):
        texture = rng.integers(0, 256, (th, tw, 3)).astype(np.uint8)
        uv = rng.uniform(-0.25, 1.25, (N, cols)).astype(np.float32)
        uv[:40, :2] = rng.integers(0, 2, (40, 2))                                   # exactly 0 and 1
        uv[40:60, :2] = np.float32(1.0) - np.float32(2.0) ** -rng.integers(1, 25, (20, 2))
        uv[60:70, :2] = [[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [0.5, -np.inf], [3e9, 0.5],
                         [0.5, -3e9], [1e38, 1e38], [-1e38, -1e38], [2.0 ** 31 / tw, 0.5], [0.5, 1 - 2.0 ** 31 / th]]
        faces_t = rng.integers(-N, N, (T, 3)).astype(np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            host = Model(vertices, faces, uv.tolist(), faces_t, texture)
        dev = DeviceModel(host)
        assert_bit_equal(dev._colors.cpu().numpy(), host._colors, f"{cols} columns, {th}x{tw}: colours")
        assert_bit_equal(dev._colors_by_triangles.cpu().numpy(), host._colors_by_triangles,
                         f"{cols} columns, {th}x{tw}: colours by triangles")
        assert_bit_equal(dev._vertices_by_triangles.cpu().numpy(), host._vertices_by_triangles, "negative face indices")


# (the 512^2 cases: tile lists longer than the resolve's LDS hash table takes — 1 024 entries on 32-pixel
# tiles, 512 on 16-pixel ones — so that some or all tiles fall back to the global pos_of look-up)
@pytest.mark.parametrize("T,res,tile", [(300_000, 1024, 0), (300_000, 2048, 0), (40_000, 512, 0),
                                        (300_000, 512, 32), (300_000, 512, 16)])
def test_tile_coherent_order_changes_nothing(oracle, T, res, tile):
    """Large models are kept in HBM sorted by screen tile (crender_plan_set_triangle_order); depth
    ties and the winner plane still speak the caller's triangle indices.  Small random triangles
    with many exact ties (coordinates snapped to a coarse grid), sorted vs unsorted vs oracle, on
    the plain and the pipelined path."""
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scenes.synthetic_triangles(T, res=res, seed=77)
    tri = (np.round(tri * 512) / 512).astype(np.float32)          # shared edges and equal depths
    f = oracle.OracleFiller(res, res, fov=45)
    f.render_arrays(tri, col, nrm)
    for presort in (True, False):
        filler = AdvancedPixelBufferFiller(res, res, fov=45, tile=tile, presort=presort, track_winner=True,
                                           pipeline=True)
        filler.render_arrays(tri, col, nrm, clear=True)
        assert (filler._order is not None) == presort
        for burst in (0, 4):
            for _ in range(burst):
                filler.render_frame()
            assert_bit_equal(filler.get_z_buffer(), f.z_buffer, f"presort={presort}: z")
            assert_bit_equal(filler.get_color_buffer(), f.color_buffer, f"presort={presort}: colour")
            assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, f"presort={presort}: normal")
            assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, f"presort={presort}: winner")


# ---- round 3: gaps named by the round-2 review -------------------------------------------------
def test_synthetic_10m_through_the_filler_matches_golden(golden):
    """configs[4] at FULL size on the path bench.py --workload synth10m takes: the filler uploads
    the numpy arrays, sorts its resident copy into tile-coherent order (presort, from 2^18 triangles
    on) and renders through k_count_wave / k_fill_wave with orig_of / pos_of — single frames and
    the swap chain — against the oracle's hashes, winner plane included."""
    from cython3dmodelrenderer_amd import scenes
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scenes.synthetic_triangles(10_000_000, res=4096)
    g = golden["scenes"]["synth10m"]
    filler = AdvancedPixelBufferFiller(4096, 4096, fov=45.0, track_winner=True, pipeline=True)
    filler.render_arrays(tri, col, nrm, clear=True)
    assert filler._order is not None, "the resident copy of a 10 M-triangle numpy model is presorted"

    def check(what):
        filler.synchronize()
        need, cap = filler.bin_usage()
        assert need <= cap, what
        got = (filler.get_z_tensor().cpu().numpy(), filler.get_color_tensor().cpu().numpy(),
               filler.get_normals_tensor().cpu().numpy(), filler.get_winner_tensor().cpu().numpy())
        assert int((got[0] < 1e6).sum()) == g["covered"], what
        assert (sha(got[0]), sha(got[1]), sha(got[2]), sha(got[3])) == (g["z"], g["c"], g["n"], g["winner"]), what

    check("render_arrays(clear=True)")
    filler.render_frame(pipelined=False)
    check("render_frame, single stream")
    for _ in range(4):
        filler.render_frame()
    check("render_frame, swap chain")


def test_overflowing_first_model_then_second_model_without_a_getter(oracle):
    """A frame whose direct bins overflow (6000 triangles around one tile corner at 1024 x 1024)
    followed by a second render_model with NO getter in between: the first frame has to be redone
    from its own inputs before the second one composites on top of it (the later call wins equal
    depths)."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(23)
    from cython3dmodelrenderer_amd import _capi
    t1, c1, n1 = random_soup(rng, 6000, 1024, size_px=(2, 6), frac_backface=0.0, margin=-0.985)
    t2, c2, n2 = scene("trex_inputs.npz")
    # the second model at the very same depth in some pixels: a copy of part of the first one
    t2 = np.concatenate([t2, t1[:500]]); c2 = np.concatenate([c2, c1[:500] * 0.5]); n2 = np.concatenate([n2, n1[:500]])
    f = oracle.OracleFiller(1024, 1024, fov=45)
    f.render_arrays(t1, c1, n1)
    f.render_arrays(t2, c2, n2)
    for numpy_inputs in (True, False):
        filler = AdvancedPixelBufferFiller(1024, 1024, fov=45)
        a = (t1, c1, n1) if numpy_inputs else (_dev(t1), _dev(c1), _dev(n1))
        b = (t2, c2, n2) if numpy_inputs else (_dev(t2), _dev(c2), _dev(n2))
        filler.render_model(_M(*a))
        filler.render_model(_M(*b))            # no getter, no synchronize in between
        assert_bit_equal(filler.get_z_buffer(), f.z_buffer, f"z (numpy inputs: {numpy_inputs})")
        assert_bit_equal(filler.get_color_buffer(), f.color_buffer, f"colour (numpy inputs: {numpy_inputs})")
        assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, f"normal (numpy inputs: {numpy_inputs})")
        assert filler._extra_flags & _capi.NO_DIRECT_BINS, "the first frame was meant to overflow the direct bins"


def test_fused_renderer_small_model_then_larger_model(oracle):
    """Renderer(on_device='fused'): render(small) then render(bigger) re-creates the filler's plan
    (T > max_T), usually at the address the old one had; the new plan must get the light again —
    a plan that kept the zero light of its creation shades the whole colour plane black."""
    from cython3dmodelrenderer_amd import Renderer
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    light = GuroIllumination([0.3, -0.2, 1])
    filler = AdvancedPixelBufferFiller(256, 256, fov=45)
    r = Renderer(filler, light, None, 256, 256, on_device="fused")
    for fixture in ("cube_inputs.npz", "trex_inputs.npz", "cube_inputs.npz", "trex_inputs.npz"):
        tri, col, nrm = scene(fixture)
        f = oracle.OracleFiller(256, 256, fov=45)
        f.render_arrays(tri, col, nrm)
        oracle.guro(f.color_buffer, f.normals_buffer, [0.3, -0.2, 1])
        img = r.render(_M(tri, col, nrm)).cpu().numpy()
        assert img.any()
        assert_bit_equal(img, f.color_buffer, f"fused render of {fixture}")


def test_presorted_model_survives_a_bin_list_regrow(oracle):
    """A presorted model (tile-coherent order) whose bin lists are far too small: the regrown plan
    must get the triangle order again — without it the winner plane reports sorted positions and
    exact-depth ties go to another triangle."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(24)
    tri, col, nrm = random_soup(rng, 20_000, 512, size_px=(2, 12), frac_backface=0.1)
    tri = np.concatenate([tri, tri[:3000]]); col = np.concatenate([col, col[:3000] * 0.25]); nrm = np.concatenate([nrm, nrm[:3000]])
    f = oracle.OracleFiller(512, 512, fov=45)
    f.render_arrays(tri, col, nrm)
    filler = AdvancedPixelBufferFiller(512, 512, fov=45, tile=32, bin_capacity=2000, direct_bins=False,
                                       presort=True, track_winner=True)
    filler.render_arrays(tri, col, nrm)
    need, cap = filler.bin_usage()
    assert cap == 2000 and need > cap and filler._order is not None
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
    assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "winner (caller's indices, ties to the highest)")
    assert filler.bin_usage()[1] >= need


def test_presort_policy_for_caller_owned_tensors(oracle):
    """Device tensors handed in by the caller are never sorted behind the caller's back: rewritten
    in place between frames, render_frame sees the new contents (also above 2^18 triangles).
    presort=True snapshots them; the cached permutation is reused while torch's version counter
    stands and redone after an in-place write."""
    import torch
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(25)
    T = (1 << 18) + 1000
    tri, col, nrm = random_soup(rng, T, 1024, size_px=(1, 5), frac_backface=0.0)
    tri2 = tri.copy(); tri2[..., 0] += np.float32(0.05) * tri2[..., 2]
    want = []
    for t in (tri, tri2):
        f = oracle.OracleFiller(1024, 1024, fov=45)
        f.render_arrays(t, col, nrm)
        want.append(f)
    dt, dc, dn = _dev(tri), _dev(col), _dev(nrm)
    filler = AdvancedPixelBufferFiller(1024, 1024, fov=45, pipeline=True)
    filler.render_arrays(dt, dc, dn, clear=True)
    assert filler._order is None and filler._inputs[0] is dt
    assert_bit_equal(filler.get_z_buffer(), want[0].z_buffer, "caller-owned tensors, first contents")
    filler.join()
    dt.copy_(torch.from_numpy(tri2))
    for _ in range(3):
        filler.render_frame()
    assert_bit_equal(filler.get_z_buffer(), want[1].z_buffer, "caller-owned tensors rewritten in place")
    assert_bit_equal(filler.get_color_buffer(), want[1].color_buffer, "colour")
    # presort="static" (the caller promises that only torch writes the tensors): snapshot + cache
    dt.copy_(torch.from_numpy(tri))
    snap = AdvancedPixelBufferFiller(1024, 1024, fov=45, presort="static")
    snap.render_arrays(dt, dc, dn, clear=True)
    first = snap._inputs
    assert snap._order is not None
    snap.render_arrays(dt, dc, dn, clear=True)
    assert snap._inputs is first, "unchanged tensors: the sorted copy is reused"
    assert_bit_equal(snap.get_z_buffer(), want[0].z_buffer, 'presort="static"')
    dt.copy_(torch.from_numpy(tri2))           # bumps the version counter
    snap.render_arrays(dt, dc, dn, clear=True)
    assert snap._inputs is not first
    assert_bit_equal(snap.get_z_buffer(), want[1].z_buffer, 'presort="static" after an in-place write')
    # presort=True: a snapshot per call, whoever wrote the tensors — here a HIP kernel through the
    # raw pointer, which torch's version counter does not see (the advisor's round-3 finding)
    dt.copy_(torch.from_numpy(tri))
    every = AdvancedPixelBufferFiller(1024, 1024, fov=45, presort=True)
    every.render_arrays(dt, dc, dn, clear=True)
    assert every._order is not None
    assert_bit_equal(every.get_z_buffer(), want[0].z_buffer, "presort=True")
    version = dt._version
    import ctypes as C
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    s3 = (C.c_double * 3)(0.01, -0.02, 0.0)
    _capi.check(lib.crender_model_shift(dt.data_ptr(), 3 * T, s3, 1,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "crender_model_shift")
    assert dt._version == version, "a write through data_ptr() is invisible to torch"
    tri3 = (tri.reshape(-1, 3) + np.array([0.01, -0.02, 0.0], np.float32)).reshape(tri.shape)
    assert np.array_equal(dt.cpu().numpy(), tri3)
    f3 = oracle.OracleFiller(1024, 1024, fov=45)
    f3.render_arrays(tri3, col, nrm)
    every.render_arrays(dt, dc, dn, clear=True)
    assert_bit_equal(every.get_z_buffer(), f3.z_buffer, "presort=True after a raw-pointer write")
    assert_bit_equal(every.get_color_buffer(), f3.color_buffer, "colour")


@pytest.mark.gpu
@pytest.mark.parametrize("presort", [True, None])
def test_presorted_filler_follows_a_device_model_through_its_transforms(oracle, presort):
    """DeviceModel rewrites its *_by_triangles arrays in place with HIP kernels (no torch version
    bump).  A filler that keeps a tile-coherent snapshot of them must notice: the model counts its
    changes (`generation`) and the filler folds the count into its keys."""
    from cython3dmodelrenderer_amd.data_structures import Model, DeviceModel
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.scenes import fit_model
    rng = np.random.default_rng(4)
    V, T = 3000, 6000
    vertices = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    host, dm = Model(vertices, faces), DeviceModel(Model(vertices, faces))
    for m in (host, dm):
        m.set_uniform_color()
        fit_model(m)
    filler = AdvancedPixelBufferFiller(512, 512, fov=45, presort=presort)
    for step, move in enumerate((None, [0.05, 0.0, 0.1], [-0.1, 0.02, 0.0])):
        if move is not None:
            dm.shift(move)
            host.shift(move)
        filler.render_model(dm, clear=True)
        if presort:
            assert filler._order is not None
        ref = oracle.OracleFiller(512, 512, fov=45)
        ref.render_model(host)
        assert_bit_equal(filler.get_z_buffer(), ref.z_buffer, f"step {step} z")
        assert_bit_equal(filler.get_color_buffer(), ref.color_buffer, f"step {step} colour")
        assert_bit_equal(filler.get_normals_buffer(), ref.normals_buffer, f"step {step} normal")
    # render_frame() on the resident model: with a snapshot (presort) it has to be retaken when the model
    # has counted a rewrite since; without one the kernels read the model's own arrays
    for pipelined in (False, True):
        f2 = AdvancedPixelBufferFiller(512, 512, fov=45, presort=presort, pipeline=pipelined)
        f2.render_model(dm, clear=True)
        for move in ([0.03, -0.04, 0.0], [0.0, 0.05, 0.05]):
            dm.shift(move)
            host.shift(move)
            f2.render_frame()
            f2.render_frame()
            ref = oracle.OracleFiller(512, 512, fov=45)
            ref.render_model(host)
            assert_bit_equal(f2.get_z_buffer(), ref.z_buffer, f"render_frame after a shift (pipelined: {pipelined}) z")
            assert_bit_equal(f2.get_color_buffer(), ref.color_buffer, "colour")
        gen = dm.generation
        dm.touch()
        assert dm.generation == gen + 1


def test_views_cross_pcie_only_when_handed_out(oracle):
    """The getters' arrays are views of pinned buffers, one per plane that was actually asked for;
    they stay live across renders (the reference's views of its own buffers) and a filler nobody
    asked a buffer of copies nothing."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    cube = scene("cube_inputs.npz")
    filler = AdvancedPixelBufferFiller(300, 400, fov=45)
    filler.render_model(_M(tri, col, nrm))
    assert not filler._host and not filler._host_pin
    c = filler.get_color_buffer()
    assert set(filler._host_pin) == {"color"} and filler._host_pin["color"].is_pinned()
    f = oracle.OracleFiller(300, 400, fov=45)
    f.render_arrays(tri, col, nrm)
    assert_bit_equal(c, f.color_buffer, "colour")
    filler.render_model(_M(*cube))
    f.render_arrays(*cube)
    assert_bit_equal(c, f.color_buffer, "the array handed out earlier shows the second render")
    assert set(filler._host_pin) == {"color"}
    z = filler.get_z_buffer()
    assert_bit_equal(z, f.z_buffer, "z handed out later")
    z[10:20] = 0.25; f.z_buffer[10:20] = 0.25       # in-place edit of a view: seen by the next render
    filler.render_model(_M(tri, col, nrm))
    f.render_arrays(tri, col, nrm)
    assert_bit_equal(z, f.z_buffer, "z after an in-place edit and a third render")
    assert_bit_equal(c, f.color_buffer, "colour after the third render")
    # numpy inputs of another size, strided inputs
    big = np.zeros((len(tri), 3, 6), np.float32)
    big[:, :, ::2] = tri
    filler.render_model(_M(big[:, :, ::2], col, nrm), clear=True)
    f.clear(); f.render_arrays(tri, col, nrm)
    assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "strided numpy input")


def test_composite_renders_never_wait_for_the_gpu(oracle, monkeypatch):
    """render_model(model) — the call Renderer.render makes (cy/renderer.py:47) — from numpy arrays, 50
    times on top of each other with no getter in between: the bin lists of every frame are verified
    from the records the raster launches leave in pinned host memory (crender_plan_poll_bin_usage),
    so the loop never asks crender_plan_last_bin_usage (a device-to-host copy and a stream
    synchronisation per call, round 4) and synchronises at most for back-pressure — when the host has
    run four frames ahead of the GPU and every staging slot is taken — never per call; the pixels are
    the oracle's."""
    import torch
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    H = W = 512
    models = [scene("trex_inputs.npz"), scene("cube_inputs.npz")]
    # (the second model nearer and smaller each time round, so that later frames win and lose pixels)
    filler = AdvancedPixelBufferFiller(H, W, fov=45, track_winner=True)
    filler.render_model(_M(*models[0]))
    filler.synchronize()                                 # plans, staging buffers: set-up is over
    filler.clear()
    calls = {"last_bin_usage": 0, "sync": 0, "poll": 0}
    lib = filler._lib
    real_usage, real_poll = lib.crender_plan_last_bin_usage, lib.crender_plan_poll_bin_usage

    def counted(name, fn):
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(lib, "crender_plan_last_bin_usage", counted("last_bin_usage", real_usage))
    monkeypatch.setattr(lib, "crender_plan_poll_bin_usage", counted("poll", real_poll))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", counted("sync", torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", counted("sync", torch.cuda.Event.synchronize))
    monkeypatch.setattr(torch.cuda, "synchronize", counted("sync", torch.cuda.synchronize))
    f = oracle.OracleFiller(H, W, fov=45)
    rng = np.random.default_rng(5)
    frames = []
    for i in range(50):
        tri, col, nrm = models[i % 2]
        tri = tri * np.float32(1.0 - 0.004 * (i // 2)) + rng.uniform(-0.02, 0.02, 3).astype(np.float32)
        frames.append((tri.astype(np.float32), col, nrm))
    for tri, col, nrm in frames:
        filler.render_model(_M(tri, col, nrm))
    assert calls["last_bin_usage"] == 0 and calls["sync"] <= len(frames) // 3, calls
    assert calls["poll"] >= 1 and len(filler._pending) <= 6
    monkeypatch.undo()
    for tri, col, nrm in frames:
        f.render_arrays(tri, col, nrm)
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z after 50 composite renders")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
    assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "normal")
    assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "winner")
    assert not filler._pending


def test_overflow_found_late_replays_the_sequence_in_order(oracle):
    """Four composite renders from numpy arrays with no getter in between, the FIRST of which
    overflows its direct bins, and later ones that hold triangles at exactly the depths of earlier
    ones (the later call must win the tie, .pyx:223): whenever the overflow is noticed — at the
    second call if the first frame's record has landed by then, at the getter otherwise — the frames
    from the overflowed one on are rendered again from their own inputs, in order."""
    from cython3dmodelrenderer_amd import _capi
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(29)
    t1, c1, n1 = random_soup(rng, 6000, 512, size_px=(2, 6), frac_backface=0.0, margin=-0.97)
    t2, c2, n2 = scene("cube_inputs.npz")
    t2 = np.concatenate([t2, t1[:700]]); c2 = np.concatenate([c2, c1[:700] * 0.5]); n2 = np.concatenate([n2, n1[:700]])
    t3, c3, n3 = t1[300:1200].copy(), c1[300:1200] * 0.25, n1[300:1200].copy()
    t4, c4, n4 = scene("trex_inputs.npz")
    t4 = np.concatenate([t4, t1[600:900]]); c4 = np.concatenate([c4, c1[600:900] * 0.125]); n4 = np.concatenate([n4, n1[600:900]])
    seq = [(t1, c1, n1), (t2, c2, n2), (t3, c3, n3), (t4, c4, n4)]
    f = oracle.OracleFiller(512, 512, fov=45)
    for a in seq:
        f.render_arrays(*a)
    filler = AdvancedPixelBufferFiller(512, 512, fov=45, tile=32, track_winner=True)
    for a in seq:
        filler.render_model(_M(*a))
    assert_bit_equal(filler.get_z_buffer(), f.z_buffer, "z")
    assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
    assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "normal")
    assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "winner")
    assert filler._extra_flags & _capi.NO_DIRECT_BINS, "the first frame was meant to overflow the direct bins"


def test_pair_bins_overflow_falls_back_to_the_scan_path(hip, oracle):
    """Scenes beyond the direct bins (more than 65 536 triangles) are binned in ONE pass into fixed-capacity
    per-tile slabs of (position, index) pairs (k_bin_wave), sized at three times the mean list.  80 000
    small triangles crowded into the middle of a 512 x 512 frame outgrow their slabs: the frame reports the
    overflow like the direct bins do (per-tile figures, crender_plan_last_frame_direct = 1), the plan goes
    back to count / scan / fill by itself, and the frame rendered again is the oracle's; the filler does
    all of that behind render_arrays.  The same scene spread over the frame fits and never leaves the
    pair bins."""
    from cython3dmodelrenderer_amd import _capi
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(41)
    H = W = 512
    for margin, overflows in ((-0.9, True), (0.1, False)):
        tri, col, nrm = random_soup(rng, 80_000, H, size_px=(2, 7), frac_backface=0.1, margin=margin)
        f = oracle_frame(oracle, tri, col, nrm, H, W)
        # C ABI: first frame through the pair bins, the redo (if any) through the scan path
        P = hip.projection_matrix(45.0, 0.1, 1000.0, H, W)
        fb = hip.FrameBuffers(H, W)
        t, c, n = _dev(tri), _dev(col), _dev(nrm)
        plan = hip.Plan(H, W, len(tri), tile=32)
        hip.render_model(plan, t, c, n, P, fb, clear=True)
        need, cap = plan.bin_usage()
        assert plan.last_frame_binning() == 2 and cap == (3 * len(tri) // 256 + 64 + 63) // 64 * 64
        assert (need > cap) == overflows, (need, cap)
        if overflows:
            hip.render_model(plan, t, c, n, P, fb, clear=True)
            need2, cap2 = plan.bin_usage()
            assert not plan.last_frame_direct() and plan.last_frame_binning() == 0 and need2 <= cap2 and cap2 != cap
        compare(fb.numpy() + (None,), f, f"pair bins, margin {margin}")
        # the filler, numpy inputs
        filler = AdvancedPixelBufferFiller(H, W, fov=45, tile=32, track_winner=True)
        filler.render_arrays(tri, col, nrm)
        assert_bit_equal(filler.get_z_buffer(), f.z_buffer, f"filler z, margin {margin}")
        assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "filler colour")
        assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "filler winner")
        assert bool(filler._extra_flags & _capi.NO_DIRECT_BINS) == overflows


def test_poll_bin_usage_c_abi(hip):
    """crender_plan_frame_ticket / crender_plan_poll_bin_usage: tickets count raster launches from 1,
    a record lands with its frame (after a synchronisation it is there), reports what
    crender_plan_last_bin_usage reports, and frames older than the ring are refused."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(31)
    tri, col, nrm = random_soup(rng, 400, 256, size_px=(30, 90), frac_backface=0.0)
    P = hip.projection_matrix(45.0, 0.1, 1000.0, 256, 256)
    fb = hip.FrameBuffers(256, 256)
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    plan = hip.Plan(256, 256, len(tri), tile=32, bin_capacity=300)
    need, cap = C.c_int64(), C.c_int64()
    assert lib.crender_plan_frame_ticket(plan.handle) == 0
    assert lib.crender_plan_poll_bin_usage(plan.handle, 1, C.byref(need), C.byref(cap)) == _capi.EINVAL
    for k in range(1, 12):
        hip.render_model(plan, t, c, n, P, fb, clear=True, direct_bins=(k % 2 == 0))
        assert lib.crender_plan_frame_ticket(plan.handle) == k
    torch.cuda.synchronize()
    want = plan.bin_usage()                       # frame 11: scan path, 300 entries are too few
    assert want[0] > want[1] == 300
    assert lib.crender_plan_poll_bin_usage(plan.handle, 11, C.byref(need), C.byref(cap)) == _capi.OK
    assert (need.value, cap.value) == want
    assert lib.crender_plan_poll_bin_usage(plan.handle, 10, C.byref(need), C.byref(cap)) == _capi.OK
    assert need.value <= cap.value and cap.value != 300          # frame 10 went through the direct bins
    assert lib.crender_plan_poll_bin_usage(plan.handle, 3, C.byref(need), C.byref(cap)) == _capi.EINVAL
    assert lib.crender_plan_poll_bin_usage(plan.handle, 12, C.byref(need), C.byref(cap)) == _capi.EINVAL


def test_usage_records_through_recycled_plans(hip, oracle):
    """A plan's bin-usage records live in a slot of a process-wide pool of pinned memory that outlives it:
    plans destroyed with their last launch still in flight (destroying does not wait), 1 100 of them one after
    another — more than the pool has slots, so slots come round again — and every so often a plan that is
    kept, whose frames must be reported with THEIR figures (a record is salted with its plan: a late store of
    a dead plan can never pass for a live plan's) and rendered right."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi
    lib = _capi.load()
    tri, col, nrm = scene("cube_inputs.npz")
    t, c, n = _dev(tri), _dev(col), _dev(nrm)
    H = W = 128
    P = hip.projection_matrix(45.0, 0.1, 1000.0, H, W)
    fb = hip.FrameBuffers(H, W)
    ref = oracle.OracleFiller(H, W, fov=45.0)
    ref.render_arrays(tri, col, nrm)
    rng = np.random.default_rng(77)
    stri, scol, snrm = random_soup(rng, 300, H, size_px=(30, 90), frac_backface=0.0)
    st, sc, sn = _dev(stri), _dev(scol), _dev(snrm)
    need, cap = C.c_int64(), C.c_int64()
    for i in range(1100):
        plan = hip.Plan(H, W, 12, tile=16)
        hip.render_model(plan, t, c, n, P, fb, clear=True)
        del plan                                  # (its launch may still be running)
        if i % 137 == 0:
            # a plan that overflows its 200-entry lists on the scan path: ITS record must say so
            keep = hip.Plan(H, W, len(stri), tile=32, bin_capacity=200)
            hip.render_model(keep, st, sc, sn, P, fb, clear=True, direct_bins=False)
            k = lib.crender_plan_frame_ticket(keep.handle)
            assert k == 1
            torch.cuda.synchronize()
            assert lib.crender_plan_poll_bin_usage(keep.handle, 1, C.byref(need), C.byref(cap)) == _capi.OK
            assert need.value > cap.value == 200, (i, need.value, cap.value)
            assert (need.value, cap.value) == keep.bin_usage()
            del keep
    plan = hip.Plan(H, W, 12, tile=16)
    hip.render_model(plan, t, c, n, P, fb, clear=True)
    torch.cuda.synchronize()
    assert lib.crender_plan_poll_bin_usage(plan.handle, 1, C.byref(need), C.byref(cap)) == _capi.OK
    assert need.value <= cap.value
    z, cb, nb, _ = fb.numpy()
    assert_bit_equal(z, ref.z_buffer, "after 1 100 recycled plans: z")
    assert_bit_equal(cb, ref.color_buffer, "after 1 100 recycled plans: colour")


def test_device_model_rotate_and_normals():
    """Row f2's expensive half on the device: Model.rotate (float64 matrix product) and the
    vertex-normal computation it triggers (model.py:175-208, 238-256).
      * against a host spelling of the SAME plain float32 operations: bit for bit (the kernels do
        what they say);
      * against the host ``Model`` (numpy + its BLAS): vertices within 1e-5 (in fact equal, the
        float64 sums round to the same float32), normals within 1e-5 EXCEPT where the discontinuous
        de-duplication test ``dot >= 1`` fell the other way on a 1-ulp difference — those vertices
        are counted, reported and bounded, not hidden."""
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    tri_fixture = scene("trex_inputs.npz")[0]
    # T-Rex-like mesh from the fixture: weld the triangle corners back into shared vertices
    flat = tri_fixture.reshape(-1, 3)
    uniq, inv = np.unique(flat.view([("", np.float32)] * 3), return_inverse=True)
    vertices = uniq.view(np.float32).reshape(-1, 3).copy()
    faces = inv.reshape(-1, 3).astype(np.int32)
    rng = np.random.default_rng(31)
    cases = [("T-Rex mesh", vertices, faces)]
    V, T = 3000, 9000
    cases.append(("random soup with repeated corners",
                  rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, V, (T, 3)).astype(np.int32)))
    flat_grid = np.stack(np.meshgrid(np.arange(40, dtype=np.float32), np.arange(40, dtype=np.float32)), -1).reshape(-1, 2)
    gv = np.concatenate([flat_grid, np.zeros((1600, 1), np.float32)], 1)      # coplanar: every face normal equal
    gi = np.arange(1600).reshape(40, 40)
    gf = np.concatenate([np.stack([gi[:-1, :-1], gi[1:, :-1], gi[:-1, 1:]], -1).reshape(-1, 3),
                         np.stack([gi[1:, 1:], gi[:-1, 1:], gi[1:, :-1]], -1).reshape(-1, 3)]).astype(np.int32)
    cases.append(("flat grid (all duplicates)", gv, gf))
    for name, vtx, fcs in cases:
        host = Model(vtx, fcs)
        dev = DeviceModel(Model(vtx, fcs))
        for angles in ([-90, 180, 0], [10, -80, 0], [33.3, 0.5, -271.0]):
            host.rotate(list(angles))
            dev.rotate(list(angles))
            dv, dn = dev._vertices.cpu().numpy(), dev._normals.cpu().numpy()
            # (1) the matrix product
            assert np.abs(dv - host._vertices).max() <= 1e-5 * max(1.0, np.abs(host._vertices).max()), name
            n_vdiff = int((dv.view(np.uint32) != host._vertices.view(np.uint32)).any(axis=1).sum())
            # (2) the kernels against the same operations spelled out on the host, from the DEVICE's vertices
            assert_bit_equal(dn, _plain_f32_vertex_normals(dv, fcs), f"{name}: device normals vs plain float32 spelling")
            # (3) against the host Model (numpy + its BLAS): no de-duplication decision may fall the
            # other way (rounds 1-3: 50-63 of T-Rex's 6 909 vertices did, with a plain float32 dot),
            # and in fact every normal is the host's, bit for bit
            err = np.abs(dn - host._normals).max(axis=1)
            flipped = int((err > 1e-5).sum())
            n_ndiff = int((dn.view(np.uint32) != host._normals.view(np.uint32)).any(axis=1).sum())
            print(f"{name} {angles}: {n_vdiff} of {len(dv)} vertices and {n_ndiff} vertex normals differ in bits, "
                  f"{flipped} de-duplication decisions fell the other way, max error {err.max():.2e}")
            assert n_vdiff <= max(2, len(dv) // 1000), name
            if numpy_dot3_is_double_accumulated():
                assert flipped == 0, (name, flipped)
                assert n_ndiff == 0, (name, n_ndiff)
            else:
                # another BLAS behind this numpy (tests/test_host_cpu.py::test_numpy_dot_of_3_vectors fails
                # first): bit parity with the host Model is unpinned, the de-duplication may flip on a
                # 1-ulp difference of the dot — bounded as in rounds 1-3
                assert flipped <= max(2, len(dv) // 50), (name, flipped)
            assert_bit_equal(dev._normals_by_triangles.cpu().numpy(), dn[fcs], f"{name}: normals by triangles")
            assert_bit_equal(dev._vertices_by_triangles.cpu().numpy(), dv[fcs], f"{name}: vertices by triangles")
            # keep the two models in step for the next rotation
            host._set_geometry(dv.copy(), host._triangles_vertices, dn.copy(), host._triangles_vertices, recalc=False)
    # lazily computed stats still match the host's after the transforms
    assert_bit_equal(dev.get_mean_vertex(), host.get_mean_vertex(), "mean vertex after rotations")


@pytest.mark.gpu
def test_device_model_trex_from_the_mesh_to_the_golden_pixels(golden):
    """Row f2 proved in pixels: the T-Rex mesh as parsed (tests/golden/trex_mesh.npz) goes through
    the README's transform ON THE DEVICE — rotate([-90, 180, 0]), rotate([10, -80, 0]), fit_model
    (README.md:62-70) — and is rendered at 1024 x 1024 straight from the device arrays: the by-triangle
    arrays equal the committed input fixture (the reference Model's, SURVEY 8c input hashes) and the
    z / colour / normal / winner planes equal golden.json's trex1024 hashes, pinned by the reference
    run."""
    import hashlib
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.scenes import fit_model, load_fixture
    from cython3dmodelrenderer_amd.scenes import GOLDEN_DIR
    with np.load(os.path.join(GOLDEN_DIR, "trex_mesh.npz")) as z:
        vertices, faces = z["vertices"], z["faces"]
    tri, col, nrm = load_fixture("trex_inputs.npz")
    if not numpy_dot3_is_double_accumulated():
        pytest.skip("this numpy's BLAS does not add float32 products in double: the device normals are pinned "
                    "against scipy-openblas 0.3.29's sdot only (parity unpinned here)")
    dm = DeviceModel(Model(vertices, faces))
    dm.rotate([-90, 180, 0])
    dm.rotate([10, -80, 0])
    fit_model(dm)
    assert_bit_equal(dm._vertices_by_triangles.cpu().numpy(), tri, "device-transformed vertices vs the input fixture")
    assert_bit_equal(dm._normals_by_triangles.cpu().numpy(), nrm, "device-computed normals vs the input fixture")
    import torch
    dm._colors_by_triangles = torch.from_numpy(col).to(dm.device)      # (texture sampling: its own test)
    dm.generation += 1
    filler = AdvancedPixelBufferFiller(1024, 1024, fov=45.0, track_winner=True)
    filler.render_model(dm, clear=True)
    g = golden["scenes"]["trex1024"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()    # noqa: E731
    assert sha(filler.get_z_buffer()) == g["z"]
    assert sha(filler.get_color_buffer()) == g["c"]
    assert sha(filler.get_normals_buffer()) == g["n"]
    filler.synchronize()
    assert sha(filler.get_winner_tensor().cpu().numpy()) == g["winner"]


@pytest.mark.parametrize("seed", range(12 * _SOAK))
def test_fuzz_a_device_model_moved_between_renders(oracle, seed):
    """Seeded sessions with a model that lives in HBM (DeviceModel): shifts and scales — HIP kernels that
    rewrite the by-triangle arrays in place and are bit-exact with the host Model's numpy — in between
    render_model calls (composite or cleared), bursts of render_frame (no swap chain, the default chain, the
    chain of depth 1; plain or with the tile-coherent snapshot ``presort=True``) that must notice the moved
    model by its generation count, and getters; the oracle renders the HOST Model's arrays, transformed by the
    same calls.  (join() before a transform while frames are in flight: the class's documented protocol.)"""
    import torch
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.scenes import GOLDEN_DIR, fit_model
    with np.load(os.path.join(GOLDEN_DIR, "trex_mesh.npz")) as z:
        vertices, faces = z["vertices"], z["faces"]
    rng = np.random.default_rng(13000 + seed)
    H = int(rng.choice([256, 384, 512])); W = int(rng.choice([256, 512]))
    kw = [{}, {"pipeline": True}, {"pipeline": True, "pipeline_depth": 1}][seed % 3]
    if seed % 4 == 3:
        kw = dict(kw, presort=True)
    hm = Model(vertices, faces)
    hm.set_uniform_color((40.0, 180.0, 250.0))
    dm = DeviceModel(Model(vertices, faces))
    dm.set_uniform_color((40.0, 180.0, 250.0))
    fit_model(hm); fit_model(dm)
    filler = AdvancedPixelBufferFiller(H, W, fov=45, **kw)
    ref = oracle.OracleFiller(H, W, fov=45.0)
    story = []

    def host_arrays():
        return hm._vertices_by_triangles, hm._colors_by_triangles, hm._normals_by_triangles

    rendered = False
    for step in range(26):
        op = str(rng.choice(["shift", "shift", "scale", "render", "render", "render clear", "frames", "frames", "check",
                             "recolour"]))
        story.append(op)
        if op == "recolour":
            # a NEW colour tensor behind the model (set_uniform_color replaces the array and counts it as a
            # rewrite): the next render_frame must render it — it rendered the old one on unsorted models
            filler.join()
            bgr = tuple(float(v) for v in rng.uniform(10, 250, 3))
            hm.set_uniform_color(bgr); dm.set_uniform_color(bgr)
        elif op in ("shift", "scale"):
            filler.join()
            if op == "shift":
                v = [float(rng.uniform(-0.08, 0.08)), float(rng.uniform(-0.08, 0.08)), float(rng.uniform(-0.1, 0.2))]
                hm.shift(v); dm.shift(v)
            else:
                c = float(rng.uniform(0.85, 1.15))
                hm.scale(c); dm.scale(c)
        elif op in ("render", "render clear"):
            if op == "render clear":
                ref.clear()
            ref.render_arrays(*host_arrays())
            filler.render_model(dm, clear=op == "render clear")
            rendered = True
        elif op == "frames":
            if not rendered:
                continue
            for _ in range(int(rng.integers(1, 5))):
                filler.render_frame()
            ref.clear()
            ref.render_arrays(*host_arrays())
        if op in ("check", "frames", "render", "render clear") and rendered:
            what = f"device-model session {seed} ({H}x{W}, {kw}), step {step} of {story}"

            def state():                # the plans' cross-frame state (crender_plan_debug_check); it synchronises
                try:
                    filler.debug_check()
                except Exception as e:
                    raise AssertionError(f"{what}: {e}") from e
            if step % 2 == 0:
                state()                 # even steps: before the pixels; odd ones: the getters meet the frames in flight
            assert_bit_equal(dm._vertices_by_triangles.cpu().numpy(), hm._vertices_by_triangles, what + ": the arrays")
            assert_bit_equal(filler.get_z_buffer(), ref.z_buffer, what + ": z")
            assert_bit_equal(filler.get_color_buffer(), ref.color_buffer, what + ": colour")
            assert_bit_equal(filler.get_normals_buffer(), ref.normals_buffer, what + ": normal")
            if step % 2:
                state()
    torch.cuda.synchronize()


@pytest.mark.parametrize("on_device_model", [False, True])
def test_renderer_normalize_model_fit(oracle, on_device_model):
    """Renderer.render(model, normalize_model=True) — the reference's fit of the model into the image
    (cy/renderer.py:40-46: scale by min(centre) / max span about the mean vertex, then shift the mean
    to (h // 2, w // 2, -min(centre))) — on the host Model and on the DeviceModel, against the oracle
    fed with the fit evaluated in numpy, statement by statement, right here."""
    from cython3dmodelrenderer_amd import Renderer
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.scenes import GOLDEN_DIR
    with np.load(os.path.join(GOLDEN_DIR, "trex_mesh.npz")) as z:
        vertices, faces = z["vertices"], z["faces"]
    H, W = 192, 256
    host = Model(vertices, faces)
    host.set_uniform_color((40.0, 180.0, 250.0))
    # ---- the fit in numpy (renderer.py:41-46 over model.py:153-160, 213-236)
    v = np.array(vertices, dtype=np.float32)
    mean = v.mean(axis=0)
    span = np.max(np.linalg.norm(v - mean, axis=-1))
    centre = (H // 2, W // 2)
    image_span = min(centre)
    coef = image_span / span
    v -= mean; v *= coef; v += mean                                   # Model.scale, keep_position
    mean = v.astype("float32").mean(axis=0)                            # _update_vertices_and_normals
    v = (v + (-mean + [centre[0], centre[1], -image_span])).astype("float32")     # Model.shift
    tri = v[faces]
    nrm = host._normals_by_triangles.copy()                            # (unchanged by scale and shift)
    col = host._colors_by_triangles.copy()
    # (the fit puts the model at z = -min(centre), in pixel units — behind the reference's own camera;
    # a wide field of view keeps part of it on screen: 1 207 pixels)
    f = oracle.OracleFiller(H, W, fov=120)
    f.render_arrays(tri, col, nrm)
    oracle.guro(f.color_buffer, f.normals_buffer, [0.2, 0.1, 1])
    assert int((f.z_buffer < 1e6).sum()) > 1000, "part of the fitted model is on screen"

    model = host
    if on_device_model:
        model = DeviceModel(host)
        model.set_uniform_color((40.0, 180.0, 250.0))
    r = Renderer(AdvancedPixelBufferFiller(H, W, fov=120), GuroIllumination([0.2, 0.1, 1]), None, H, W)
    img = r.render(model, normalize_model=True)
    got_tri = model._vertices_by_triangles
    got_tri = got_tri.cpu().numpy() if on_device_model else got_tri
    assert_bit_equal(got_tri, tri, "fitted vertices by triangles")
    assert_bit_equal(img, f.color_buffer, "shaded colour of the fitted model")
    assert_bit_equal(r.pixel_buffer_filler.get_z_buffer(), f.z_buffer, "z of the fitted model")


def test_device_model_stats_are_lazy():
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    rng = np.random.default_rng(32)
    vtx = rng.standard_normal((500, 3)).astype(np.float32)
    fcs = rng.integers(0, 500, (900, 3)).astype(np.int32)
    host, dev = Model(vtx, fcs), DeviceModel(Model(vtx, fcs))
    assert not dev._stats_valid
    for m in (host, dev):
        m.shift(np.array([1.0, 2.0, 3.0], np.float32))
        m.shift([0.5, 0.25, -1.0])
    assert not dev._stats_valid                     # two shifts: no serial mean pass yet
    for m in (host, dev):
        m.scale(0.5)                                # keep_position: needs the mean of the shifted vertices
    assert_bit_equal(dev._vertices.cpu().numpy(), host._vertices, "vertices after shift, shift, scale")
    assert_bit_equal(dev.get_mean_vertex(), host.get_mean_vertex(), "mean vertex")


def test_device_model_stats_on_a_model_of_2_pow_24_vertices():
    """The mean vertex is numpy's sequential float32 sum (rows one after another, the first row the
    start value) divided by the count in float64: pinned above 2^24 vertices too, where the count
    is no float32 any more and the accumulator has long stopped taking in small terms — and the
    serial kernel has to stay usable (loads batched ahead of the additions)."""
    import time
    import torch
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    rng = np.random.default_rng(33)
    V = (1 << 24) + 5
    vtx = (rng.standard_normal((V, 3), dtype=np.float32) * np.float32(3.0) + np.array([100.0, -7.0, 0.01], np.float32))
    vtx[0] = [-0.0, 5.0, -3.0]
    fcs = rng.integers(0, V, (64, 3)).astype(np.int32)
    host = Model.__new__(Model)                      # (the host constructor's vertex normals are beside the point)
    mean = vtx.mean(axis=0)
    span = np.max(np.linalg.norm(vtx - mean, axis=-1))
    dev = DeviceModel.__new__(DeviceModel)
    from cython3dmodelrenderer_amd import _capi
    dev._lib = _capi.load(); dev.device = torch.device("cuda:0")
    dev._vertices = torch.from_numpy(vtx).to("cuda:0")
    dev._stats = torch.zeros(4, dtype=torch.float32, device="cuda:0")
    dev._stats_valid = False; dev._stats_host = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got_mean, got_span = dev.get_mean_vertex(), dev.get_max_span()
    dt = time.perf_counter() - t0
    assert_bit_equal(got_mean, mean, "mean of 2^24 + 5 vertices")
    assert np.float32(got_span).view(np.uint32) == np.float32(span).view(np.uint32)
    print(f"crender_model_stats: {dt * 1e3:.1f} ms for {V} vertices")
    assert dt < 5.0, f"crender_model_stats took {dt:.1f} s for {V} vertices"
    del host, fcs


def test_device_model_transformed_between_pipelined_frames(oracle):
    """The documented protocol for changing a resident DeviceModel under a swap chain: join, transform
    (the kernels rewrite the arrays in place on the current stream), hand the model to render_model
    again (re-binds every slot: what was binned ahead from the old vertices is dropped), go on."""
    from cython3dmodelrenderer_amd.data_structures import DeviceModel, Model
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.scenes import fit_model
    rng = np.random.default_rng(41)
    V, T = 900, 2500
    vertices = rng.standard_normal((V, 3)).astype(np.float32)
    faces = rng.integers(0, V, (T, 3)).astype(np.int32)
    host, dev = Model(vertices, faces), DeviceModel(Model(vertices, faces))
    for m in (host, dev):
        m.set_uniform_color()
        fit_model(m)
    filler = AdvancedPixelBufferFiller(256, 256, fov=45, pipeline=True)
    for step, move in enumerate(([0.0, 0.0, 0.0], [0.2, -0.1, 0.3], [-0.35, 0.2, 0.1])):
        filler.join()
        for m in (host, dev):
            m.shift(np.array(move, np.float32))
        filler.render_model(dev, clear=True)
        for _ in range(5):
            filler.render_frame()
        f = oracle.OracleFiller(256, 256, fov=45)
        f.render_model(host)
        assert_bit_equal(filler.get_z_buffer(), f.z_buffer, f"z after move {step}")
        assert_bit_equal(filler.get_color_buffer(), f.color_buffer, f"colour after move {step}")


def test_swap_chain_with_its_own_tile_size(oracle):
    """The swap chain picks 32-pixel tiles for its plans (throughput) beside the single-frame plan's
    16-pixel tiles (latency) in one filler; every frame of either kind is the oracle's frame."""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("trex_inputs.npz")
    f = oracle.OracleFiller(1024, 1024, fov=45)
    f.render_arrays(tri, col, nrm)
    filler = AdvancedPixelBufferFiller(1024, 1024, fov=45, pipeline=True, track_winner=True)
    filler.render_arrays(tri, col, nrm, clear=True)
    for burst, pipelined in ((6, True), (1, False), (9, True)):
        for _ in range(burst):
            filler.render_frame(pipelined=pipelined)
        assert_bit_equal(filler.get_z_buffer(), f.z_buffer, f"z ({burst} frames, pipelined={pipelined})")
        assert_bit_equal(filler.get_color_buffer(), f.color_buffer, "colour")
        assert_bit_equal(filler.get_normals_buffer(), f.normals_buffer, "normal")
        assert_bit_equal(filler.get_winner_tensor().cpu().numpy(), f.winner, "winner")
    assert filler._pipe is not None and filler._pipe.lookahead and filler._pipe.tile == 32


@pytest.mark.parametrize("name,fixture,res", [("bunny4096", "bunny_inputs.npz", 4096), ("trex8192", "trex_inputs.npz", 8192)])
def test_full_size_idempotence_and_strips_through_the_pixel_owners(hip, golden, name, fixture, res):
    """Size-independent properties at BASELINE.json's full sizes on the path these frames take (32-pixel
    tiles, pixel owners): drawing the same model again on top of the finished frame (compositing: every
    fragment ties with the prior value and must overwrite it with identical bits) changes nothing, and
    the frame assembled from 5 ragged row strips equals the whole one — all against the golden hashes."""
    tri, col, nrm = scene(fixture)
    g = golden["scenes"][name]
    got = gpu_frame(hip, tri, col, nrm, res, res, mode="fused", clear=True)
    assert (sha(got[0]), sha(got[1]), sha(got[2])) == (g["z"], g["c"], g["n"])
    twice = gpu_frame(hip, tri, col, nrm, res, res, mode="fused", prior=got[:3])
    assert (sha(twice[0]), sha(twice[1]), sha(twice[2])) == (g["z"], g["c"], g["n"]), "idempotence"
    cuts = [0, res // 7 + 3, res // 3, res // 2 + 17, res - 29, res]
    strips = list(zip(cuts, cuts[1:]))
    parts = gpu_frame(hip, tri, col, nrm, res, res, mode="fused", strips=strips, clear=True)
    assert (sha(parts[0]), sha(parts[1]), sha(parts[2])) == (g["z"], g["c"], g["n"]), "ragged strips"


def _bench_line(args, nproc, timeout=600):
    """Run bench.py as the driver does for N > 1 — a fresh child, `python -m torch.distributed.run
    --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...` —
    and return rank 0's one JSON line."""
    import json, socket, subprocess, sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
           "--gpus", str(nproc)] + args
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line from rank 0, got {len(lines)}: {out.stdout[-2000:]}"
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_launch_contract_two_ranks_strips():
    """The N > 1 contract of bench.py end to end, so that the first multi-GPU scaling run measures
    RCCL and not argument parsing: two ranks on the one GPU (gloo carries the timings; --no-gather
    because gloo cannot all-gather device strips in place), north_star's layout (row strips of
    T-Rex 8192^2, strong scaling), the CPU baseline beside it (--full)."""
    d = _bench_line(["--full", "--backend", "gloo", "--no-gather", "--steps", "3", "--warmup", "1"], 2)
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert d["scaling"] == "strong" and d["config"]["workload"] == "trex8192"
    assert d["metric"].startswith("frames") and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"]
    for key in ("ms_per_step_without_exchange", "cpu_baseline", "strong_scaling_reference", "roofline"):
        assert key in d, key
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] == "port" and "1" in cb["frames_per_s_by_threads"]
    assert len(cb["frames_per_s_by_threads"]) >= 1 + sum(t <= cb["host_cpus"] for t in (8, 16))
    assert cb["best"]["frames_per_s"] == max(cb["frames_per_s_by_threads"].values())
    assert cb["omp"]["OMP_PROC_BIND"] == "close"           # in the baseline's own process, and only there:
    assert d["submit_thread_affinity_cpus_min_over_ranks"] > 2, "a rank's submitting thread was bound to a core"
    ex = d["exchange"]                                      # the line explains its own scaling
    assert ex["kind"] is None and ex["exchange_bytes_received_per_rank"] == 0          # (--no-gather)
    assert ex["bytes_received_per_rank_by_choice"] == {"planes": 28 * 4096 * 8192, "color": 12 * 4096 * 8192,
                                                       "present": 3 * 4096 * 8192}
    assert abs(ex["exchange_ms"] - (d["ms_per_step"] - d["ms_per_step_without_exchange"])) < 1e-9
    assert "speedup_lone_frame" in d and d["csrc_sha16"]
    wk = d["weak_scaling_frames"]                           # and the weak-scaling curve's point from the same run
    assert wk["workload"] == "trex1024" and wk["n_gpus"] == 2 and wk["scaling"] == "weak" and wk["value"] > 0
    assert d["config"]["raster_path"]["asked"] == "auto"


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_launch_contract_two_ranks_frames():
    """--mode frames: every rank its own full frames, no collective in the data path (weak scaling); --full."""
    d = _bench_line(["--full", "--backend", "gloo", "--mode", "frames", "--workload", "trex1024", "--steps", "5",
                     "--warmup", "2", "--no-api-calls"], 2)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["workload"] == "trex1024"
    assert d["value"] > 0 and "cpu_baseline" in d and "roofline" in d
    assert d["submit_thread_affinity_cpus_min_over_ranks"] > 2, "a rank's submitting thread was bound to a core"
    assert "exchange" not in d and d["speedup_vs_best_cpu_column"] <= d["speedup_vs_cpu_baseline"] * 1.0000001


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_plain_line_and_dumped_outputs(oracle, tmp_path):
    """The driver's command, `bench.py --gpus 1 --steps K --warmup W`, prints the headline alone (no figure
    that takes passes of its own), and with --dump-outputs writes what the last timed step computed: the
    whole T-Rex 1024^2 frame in float32, bit for bit the oracle's."""
    import json, subprocess, sys
    from cython3dmodelrenderer_amd import scenes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=540)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "frames/sec" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 7 and d["warmup"] == 2 and d["config"]["workload"] == "trex1024"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6
    for key in ("kernel_ms", "ms_per_frame_single_stream", "roofline", "cpu_baseline", "api_call"):
        assert key not in d, key
    assert d["outputs"]["pixels"] == "all" and d["outputs"]["arrays"]["color"] == [1024, 1024, 3]
    ref = oracle.OracleFiller(1024, 1024, fov=45)
    ref.render_arrays(*scenes.load_fixture("trex_inputs.npz"))
    for name, want in (("z", ref.z_buffer), ("color", ref.color_buffer), ("normals", ref.normals_buffer)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32
        assert_bit_equal(got, want, name)


@pytest.mark.gpu
def test_normal_z_array_feeds_the_back_face_test(oracle):
    """crender_plan_set_normal_z: the scan path's binning pass takes the normals' z components from the
    array of their own (the filler makes it with its tile-coherent copy).  Same frame as without it;
    and the array is what is read: with every component +1 in it, everything is culled."""
    import ctypes as C
    import torch
    from cython3dmodelrenderer_amd import _capi
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    rng = np.random.default_rng(8)
    T = (1 << 18) + 77
    tri, col, nrm = random_soup(rng, T, 1024, size_px=(1, 6), frac_backface=0.3)
    ref = oracle.OracleFiller(1024, 1024, fov=45)
    ref.render_arrays(tri, col, nrm)
    filler = AdvancedPixelBufferFiller(1024, 1024, fov=45)
    filler.render_arrays(tri, col, nrm, clear=True)
    assert filler._order is not None and filler._order[2].shape == (T, 3)
    assert_bit_equal(filler._order[2].cpu().numpy(), filler._inputs[2].cpu().numpy()[:, :, 2], "nz = nrm[:, :, 2]")
    assert_bit_equal(filler.get_z_buffer(), ref.z_buffer, "z with the components apart")
    assert_bit_equal(filler.get_normals_buffer(), ref.normals_buffer, "normal")
    plain = AdvancedPixelBufferFiller(1024, 1024, fov=45, presort=False)      # caller's order, normals read in place
    plain.render_arrays(tri, col, nrm, clear=True)
    assert plain._order is None
    assert_bit_equal(plain.get_z_buffer(), ref.z_buffer, "z without")
    filler._order[2].fill_(1.0)                  # every triangle now "faces away"
    filler.render_frame(pipelined=False)
    assert float(filler.get_z_buffer().min()) == 1e6, "the back-face test read the array it was given"


# ---- the raster kernels of a 32-pixel plan (crender_plan_set_raster_path): each exact on every tile ----------
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name,fixture,res", SCENES)
@pytest.mark.parametrize("mode", ["fused", "fused-scan", "split"])
def test_every_raster_kernel_renders_every_scene(hip, oracle, golden, name, fixture, res, mode, path):
    tri, col, nrm = scene(fixture)
    f = oracle_frame(oracle, tri, col, nrm, res, res)
    got = gpu_frame(hip, tri, col, nrm, res, res, mode=mode, tile=32, raster_path=path)
    compare(got, f, f"{name}/{mode}/path {path}")
    g = golden["scenes"][name]
    assert (sha(got[0]), sha(got[1]), sha(got[2]), sha(got[3])) == (g["z"], g["c"], g["n"], g["winner"])


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("seed,T,H,W,px,kw", [
    (3, 5000, 256, 256, (0.3, 4), {}),                # tiny records through the pixel owners
    (5, 300, 512, 512, (100, 600), {}),               # huge ones
    (6, 3000, 333, 517, (0.5, 200), {"margin": 1.0}), # mixed sizes, ragged frame
    (8, 9000, 96, 64, (1, 30), {}),                   # six tiles, ~2 000 records each: lists of many batches
])
@pytest.mark.parametrize("how", ["clear", "composite", "strips"])
def test_every_raster_kernel_on_soups_composites_and_strips(hip, oracle, seed, T, H, W, px, kw, how, path):
    """The pixel owners' kernel takes EVERY tile its plan holds: lists of more than one batch (the pixels'
    running minimum stays in registers across the batches, each batch stores what it won), small records,
    frames that composite onto a prior buffer, row strips that cut tiles."""
    rng = np.random.default_rng(seed)
    tri, col, nrm = random_soup(rng, T, max(H, W), size_px=px, **kw)
    prior = None
    if how == "composite":
        prior = (rng.uniform(0.5, 2.5, (H, W)).astype(np.float32),
                 rng.uniform(0, 255, (H, W, 3)).astype(np.float32), rng.standard_normal((H, W, 3)).astype(np.float32))
        prior[0][::7, ::5] = np.nan                   # a NaN already in the buffer loses to every fragment
    strips = [(0, 37), (37, H - 13), (H - 13, H)] if how == "strips" else None
    f = oracle_frame(oracle, tri, col, nrm, H, W, strips=strips, prior=prior)
    for mode in ("fused", "fused-scan"):
        got = gpu_frame(hip, tri, col, nrm, H, W, mode=mode, tile=32, strips=strips, prior=prior,
                        clear=(how == "clear"), raster_path=path)
        compare(got, f, f"soup{seed}/{how}/{mode}/path {path}", check_winner=(how != "composite"))


def test_plans_pick_their_raster_kernel_from_what_their_frames_count(hip, oracle):
    """crender_plan_set_raster_path(-1), the default: a plan's first launches go by the triangle count per tile,
    later ones by the size classes the tiles themselves counted (the launch's usage record carries the sums of
    the launch before it).  bunny 2048^2 — 7 triangles per tile, but large ones — starts on the general kernel
    and moves to the pixel owners with its third frame; T-Rex 1024^2 on 32-pixel tiles stays; the cube (12
    triangles) starts with the owners.  Whatever the kernel, the pixels are the oracle's."""
    for fixture, res, want in (("bunny_inputs.npz", 2048, [0, 0, 1, 1]), ("trex_inputs.npz", 1024, [0, 0, 0, 0]),
                               ("cube_inputs.npz", 256, [1, 1, 1, 1])):
        tri, col, nrm = scene(fixture)
        f = oracle_frame(oracle, tri, col, nrm, res, res)
        P = hip.projection_matrix(45.0, 0.1, 1000.0, res, res)
        t, c, n = _dev(tri), _dev(col), _dev(nrm)
        plan = hip.Plan(res, res, len(tri), tile=32)
        paths = []
        for k in range(4):
            fb = hip.FrameBuffers(res, res)
            hip.render_model(plan, t, c, n, P, fb, clear=True)
            got = fb.numpy()                          # (synchronises: the launch's record has landed)
            paths.append(plan.last_raster_path())
            compare(got + (None,), f, f"{fixture} frame {k} on kernel {paths[-1]}")
        assert paths == want, (fixture, paths)
        plan.set_raster_path(0)                       # the caller's word goes first, and -1 hands the choice back
        fb = hip.FrameBuffers(res, res)
        hip.render_model(plan, t, c, n, P, fb, clear=True)
        compare(fb.numpy() + (None,), f, "forced general")
        assert plan.last_raster_path() == 0
        plan.set_raster_path(-1)
        hip.render_model(plan, t, c, n, P, fb, clear=True)
        fb.numpy()
        assert plan.last_raster_path() == want[-1]


def test_a_swap_chain_shares_what_one_plan_learnt(oracle):
    """The plans of a swap chain (two per slot with look-ahead) render the same stream of frames: the size class one
    of them has read from its records is every plan's from its next launch on (crender_pipeline_frame).  (A plan
    learns with its third launch: its second launch's record carries what its first counted.  Six plans take
    turns: the first of them knows at the chain's thirteenth frame, all of them one round later.)"""
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    tri, col, nrm = scene("bunny_inputs.npz")
    res = 2048
    f = oracle_frame(oracle, tri, col, nrm, res, res)
    filler = AdvancedPixelBufferFiller(res, res, fov=45.0, pipeline=True, pipeline_depth=3, track_winner=True)
    filler.render_arrays(tri, col, nrm, clear=True)
    filler.synchronize()
    for k in range(27):
        filler.render_frame()
        if k % 3 == 2:
            filler.synchronize()
            assert_bit_equal(filler.get_z_tensor().cpu().numpy(), f.z_buffer, f"frame {k}: z")
            assert_bit_equal(filler.get_color_tensor().cpu().numpy(), f.color_buffer, f"frame {k}: colour")
    filler.synchronize()
    paths = filler.last_raster_paths()
    assert len(paths) == 1 + 6 and paths[1:] == [1] * 6, paths
    assert_bit_equal(filler.get_normals_tensor().cpu().numpy(), f.normals_buffer, "normal")
