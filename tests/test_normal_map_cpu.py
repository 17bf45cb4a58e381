"""Normal mapping without a GPU: the two entries' declarations against the binding and the build tables, their argument
checks, ``nmap_ref.from_height`` against a plain loop and the float64 unit normal, and the host model the GPU tests
compare with (tests/nmap_ref.py) pinned on the oracle's frames: by counts, by identities, by the sign convention on a
camera-facing quad and against itself in float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mip_ref
import nmap_ref
import pass_scenes
from pass_scenes import Frame, capi, trex_fixture, trex_uv  # noqa: F401 (fixtures)
from util import assert_bit_equal, other_symbols, own_unit_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crender_nmap_from_height", "crender_nmap_shade")


# ---- 1. the host side of the ABI -------------------------------------------------------------------------------------

def test_nmap_symbols_are_declared_bound_and_exported(capi):
    header = open(os.path.join(ROOT, "include", "crender_nmap.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["nmap"]) == set(ENTRIES)
    assert not declared & other_symbols(capi, "nmap")
    L = capi.load()
    _vp, _i32, _i64, _u32, _f32p, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.POINTER(C.c_float), C.c_float
    want = {"crender_nmap_from_height": [_vp, _i32, _i32, _f, _u32, _vp, _vp],
            "crender_nmap_shade": [_vp, _vp, _i64, _vp, _f32p, _vp, _vp, _i32, _i32, _f, _vp, _i32, _i32, _i32, _i32, _u32, _vp]}
    for name in ENTRIES:
        res, args = capi.UNIT_SIGNATURES["nmap"][name]
        assert res == C.c_int and args == want[name] == getattr(L, name).argtypes, name
        decl = re.search(r"CRENDER_API int " + name + r"\((.*?)\);", header, re.S).group(1).split(",")
        assert len(decl) == len(args), name
        # the floats of the declaration are the table's
        floats = [i for i, a in enumerate(decl) if re.match(r"\s*float \w+$", a)]
        assert floats == [i for i, a in enumerate(args) if a is _f] == ([3] if name == ENTRIES[0] else [9]), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert set(ENTRIES) <= set(re.findall(r" T (crender_\w+)", out))
    flags = dict(re.findall(r"(CRENDER_NMAP_\w+) = (\d+)u", header))
    assert (int(flags["CRENDER_NMAP_PERSPECTIVE"]), int(flags["CRENDER_NMAP_BILINEAR"]), int(flags["CRENDER_NMAP_CHAIN"])) == \
        (capi.NMAP_PERSPECTIVE, capi.NMAP_BILINEAR, capi.NMAP_CHAIN) == (1, 2, 4)
    assert int(re.search(r"#define CRENDER_NMAP_WRAP (\d+)u", header).group(1)) == capi.NMAP_WRAP == 1
    assert capi.ABI_VERSION == 6


def test_nmap_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit = new = own_unit_source(_build, "nmap", "normal_map.hip", "crender_nmap.h")
    assert unit.count("// ---- normal mapping") == 1 and new.count("namespace {") == 1 and new.count('extern "C" {') == 1
    # the mip unit's headers stay its own: what the pass needs of them is restated
    assert "mip_sample.h\"" not in unit and "crender_mip.h\"" not in unit
    assert not re.search(r"#include[^\n]*(mip_sample|crender_mip)", unit)
    # the kernels take the passes' frame from the shared header
    for name in ("k_nmap_shade", "k_nmap_from_height"):
        assert unit.index("// ---- normal mapping") < unit.index("void " + name) < unit.index("int crender_nmap_from_height("), name
    for name in ("winner_triangle(", "winner_pixel(", "barycentric(", "bilinear(", "make_proj(", "wave_any(", "pass_grid(",
                 "frame_checks(", "rows_check(", "arg_error("):
        assert name in new and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    assert "project_vertex(" not in unit and "gather_corners(" not in unit
    # six instances of the pass
    assert len(set(re.findall(r"k_nmap_shade<(?:true|false), kNmap\w+>", new))) == 6


# ---- 2. argument errors ----------------------------------------------------------------------------------------------

def test_nmap_from_height_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")

    def make(h=fake, mh=4, mw=4, scale=1.0, flags=0, out=fake):
        return L.crender_nmap_from_height(h, mh, mw, scale, flags, out, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(h=None), dict(out=None)):
        assert make(**kw) == E and "d_height or d_map is NULL" in text(), kw
    for kw in (dict(mh=0), dict(mw=0), dict(mh=-3), dict(mh=65536), dict(mw=65536), dict(mw=2 ** 31 - 1)):
        assert make(**kw) == E and "mh or mw is not 1 .. 65535" in text(), kw
    for bad in (nan, inf, -inf):
        assert make(scale=bad) == E and "scale is not finite" in text(), bad
    for flags in (2, 4, 3, 0x80000000):
        assert make(flags=flags) == E and "unknown flag bits" in text(), flags
    assert text().startswith("crender_nmap_from_height: ")
    # the documented order: pointers, size, scale, flags
    assert make(h=None, mh=0) == E and "NULL" in text()
    assert make(mh=0, scale=nan) == E and "mh or mw" in text()
    assert make(scale=nan, flags=2) == E and "scale" in text()


def test_nmap_shade_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = (C.c_float * 16)(*([0.0] * 16))
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first or has T == 0
    nan, inf = float("nan"), float("inf")

    def shade(win=fake, tri=fake, T=4, pos_of=None, P=P, uv=fake, nmap=fake, mh=8, mw=8, strength=1.0, nrm=fake, H=8, W=8,
              y0=0, y1=8, flags=0):
        return L.crender_nmap_shade(win, tri, T, pos_of, P, uv, nmap, mh, mw, strength, nrm, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(P=None), dict(nmap=None), dict(nrm=None)):
        assert shade(**kw) == E and "d_winner, P16, d_map or d_normal is NULL" in text(), kw
    assert shade(T=-1) == E and "T is negative" in text()
    for kw in (dict(tri=None), dict(uv=None), dict(tri=None, uv=None)):
        assert shade(**kw) == E and "d_tri or d_uv is NULL with T > 0" in text(), kw
    for kw in (dict(H=0), dict(W=-2)):
        assert shade(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert shade(**kw) == E and "rows outside the frame" in text(), kw
    for kw in (dict(mh=0), dict(mw=0), dict(mh=-1), dict(mh=65536), dict(mw=65536)):
        assert shade(**kw) == E and "mh or mw is not 1 .. 65535" in text(), kw
    for bad in (nan, inf, -inf):
        assert shade(strength=bad) == E and "strength is not finite" in text(), bad
    for flags in (8, 16, 0x80000000, 8 | 1):
        assert shade(flags=flags) == E and "unknown flag bits" in text(), flags
    for flags in (6, 7):
        assert shade(flags=flags) == E and "CRENDER_NMAP_CHAIN with CRENDER_NMAP_BILINEAR" in text(), flags
    assert text().startswith("crender_nmap_shade: ")
    # the documented order, pair by pair
    assert shade(win=None, T=-1) == E and "is NULL" in text() and "T >" not in text()
    assert shade(T=-1, H=0) == E and "T is negative" in text()
    assert shade(tri=None, H=0) == E and "NULL with T > 0" in text()
    assert shade(H=0, y0=-1) == E and "H or W" in text()
    assert shade(y0=-1, mh=0) == E and "rows" in text()
    assert shade(mh=0, strength=nan) == E and "mh or mw" in text()
    assert shade(strength=nan, flags=8) == E and "strength" in text()
    assert shade(flags=8 | 6) == E and "unknown flag bits" in text()
    # bad arguments are refused without triangles too; a valid call without triangles launches nothing
    assert shade(T=0, flags=6) == E and shade(T=0, mh=0) == E and shade(T=0, nrm=None) == E
    for flags in (0, 1, 2, 3, 4, 5):
        assert shade(T=0, tri=None, uv=None, flags=flags) == capi.OK, flags
    assert shade(T=0, strength=0.0, mh=65535, mw=1, y0=7, y1=8) == capi.OK


# ---- 3. from_height ----------------------------------------------------------------------------------------------------

def _loop(h, scale, wrap):
    """crender_nmap_from_height texel by texel, in numpy float32 scalars."""
    d = np.float32
    mh, mw = h.shape
    out = np.zeros((mh, mw, 3), np.uint8)
    k = d(scale) / d(255.0)

    def at(r, c):
        if wrap:
            return int(h[r % mh, c % mw])
        return int(h[min(max(r, 0), mh - 1), min(max(c, 0), mw - 1)])
    for r in range(mh):
        for c in range(mw):
            gx = d(at(r, c + 1) - at(r, c - 1)) * k
            gy = d(at(r - 1, c) - at(r + 1, c)) * k
            ln = np.sqrt(d(d(gx * gx) + d(gy * gy)) + d(1))
            for j, v in enumerate((-gx / ln, -gy / ln, d(1) / ln)):
                out[r, c, j] = int(min(max(np.rint(d(v * d(127)) + d(128)), 0), 255))
    return out


def test_from_height_flat_and_tiny_maps():
    flat = np.array(nmap_ref.FLAT, np.uint8)
    for h in (np.zeros((5, 7), np.uint8), np.full((3, 3), 255, np.uint8), np.full((1, 1), 90, np.uint8)):
        for wrap in (False, True):
            for scale in (1.0, -40.0, 0.0):
                assert (nmap_ref.from_height(h, scale, wrap) == flat).all(), (h.shape, wrap, scale)
    # 1 x 7: no gradient along v, whatever the rows' neighbours are; along u the clamp halves the step at the two ends
    row = np.uint8([[0, 40, 80, 120, 160, 200, 240]])
    out = nmap_ref.from_height(row, 4.0)
    assert out.shape == (1, 7, 3) and (out[..., 1] == 128).all()
    assert (out[0, 1:-1] == out[0, 1]).all() and out[0, 0, 0] > out[0, 1, 0] and (out[0, 0] == out[0, -1]).all()
    assert (out[..., 0] < 128).all() and (out[..., 2] < 255).all()
    assert_bit_equal(out, _loop(row, 4.0, False), "1 x 7")
    # wrapped, the two ends see the fall from 240 to 0 and tilt the other way
    wrapped = nmap_ref.from_height(row, 4.0, wrap=True)
    assert (wrapped[0, 1:-1] == out[0, 1:-1]).all() and wrapped[0, 0, 0] > 128 and wrapped[0, -1, 0] > 128
    assert_bit_equal(wrapped, _loop(row, 4.0, True), "1 x 7, wrapped")


def test_from_height_wrap_against_clamp_on_a_ramp():
    ramp = np.tile((np.arange(16) * 10).astype(np.uint8), (6, 1))
    a, b = nmap_ref.from_height(ramp, 2.0), nmap_ref.from_height(ramp, 2.0, wrap=True)
    assert (a[:, 1:-1] == b[:, 1:-1]).all() and (a[:, [0, -1]] != b[:, [0, -1]]).any()
    assert (a[..., 0] < 128).all()                            # uphill along u: every normal leans back along -u
    assert (b[:, [0, -1], 0] > 128).all()                     # the seam is a cliff the other way
    down = nmap_ref.from_height(ramp.T.copy(), 2.0)           # the height grows with the ROW: downhill along v
    assert (down[..., 1] > 128).all() and (down[..., 0] == 128).all()


def test_from_height_is_the_loop_and_a_unit_normal():
    rng = np.random.default_rng(5)
    h = rng.integers(0, 256, (9, 11), dtype=np.uint8)
    for scale, wrap in ((1.0, False), (1.0, True), (-7.5, False), (300.0, True), (1e-3, False)):
        got = nmap_ref.from_height(h, scale, wrap)
        assert got.dtype == np.uint8 and got.shape == (9, 11, 3)
        assert_bit_equal(got, _loop(h, scale, wrap), f"scale {scale}, wrap {wrap}")
        # within one byte step of the float64 unit normal of the same differences
        hp = np.pad(h.astype(np.float64), 1, mode="wrap" if wrap else "edge")
        gx = (hp[1:-1, 2:] - hp[1:-1, :-2]) * scale / 255.0
        gy = (hp[:-2, 1:-1] - hp[2:, 1:-1]) * scale / 255.0
        n = np.stack([-gx, -gy, np.ones_like(gx)], 2) / np.sqrt(gx * gx + gy * gy + 1.0)[..., None]
        assert np.abs(nmap_ref.decode(got) - n).max() <= 1.0 / 127.0
    # an overflowing scale: the NaN of inf / inf gives byte 0, never an undefined conversion
    big = nmap_ref.from_height(h, 3e38)
    assert set(np.unique(big)) <= {0, 128, 255}


# ---- 4. the model on the oracle's frames -------------------------------------------------------------------------------

class _Frame(Frame):
    def run(self, uv, nmap, filter="bilinear", perspective=True, strength=1.0, normals=None, **kw):
        return nmap_ref.normal_map_pass(self.cam.normals_buffer if normals is None else normals, self.cam.winner, self.tri,
                                        self.cam.proj_mat, uv, nmap, perspective, filter, strength, **kw)


trex = trex_fixture(_Frame)


@pytest.fixture(scope="module")
def nmap64():
    m = nmap_ref.from_height(pass_scenes.texture(8, 64, 64)[:, :, 0], 1.0)
    assert [(int(m[..., j].min()), int(m[..., j].max())) for j in range(3)] == [(39, 216), (40, 217), (205, 255)]
    assert not (m == np.array(nmap_ref.FLAT, np.uint8)).all(2).any()
    return m


def _guro_changed(oracle, a, b):
    base = np.full(a.shape, 200.0, np.float32)
    ga, gb = (oracle.guro(base.copy(), np.ascontiguousarray(n), pass_scenes.LIGHT) for n in (a, b))
    return int((ga.view(np.uint32) != gb.view(np.uint32)).any(2).sum())


@pytest.mark.parametrize("filter,lit", [("nearest", 15666), ("bilinear", 15654), ("trilinear", 15653)])
def test_the_counts_on_trex(oracle, trex, trex_uv, nmap64, filter, lit):
    counts = {}
    out = trex.run(trex_uv[3], nmap64, filter, counts=counts)
    assert out.dtype == np.float32 and not np.isnan(out).any()
    mask = counts.pop("mask")
    assert counts == dict(covered=15801, written=15801, det_zero=0, mirrored=730, flipped=730)
    assert (mask == trex.covered).all()
    assert_bit_equal(out[~trex.covered], trex.cam.normals_buffer[~trex.covered], "the background is not written")
    assert _guro_changed(oracle, out, trex.cam.normals_buffer) == lit


def test_identities_bit_for_bit(trex, trex_uv, nmap64):
    uv = trex_uv[3]
    flat = np.broadcast_to(np.array(nmap_ref.FLAT, np.uint8), (5, 9, 3))
    for filter in nmap_ref.FILTERS:
        counts = {}
        assert_bit_equal(trex.run(uv, flat, filter, counts=counts), trex.cam.normals_buffer, f"a flat map, {filter}")
        assert counts["written"] == 0 and counts["covered"] == 15801
        for strength in (0.0, -0.0):
            assert_bit_equal(trex.run(uv, nmap64, filter, strength=strength, counts=counts), trex.cam.normals_buffer,
                             f"strength {strength}, {filter}")
            assert counts["written"] == 0
    # degenerate uv (all three corners alike, or on one line) and dead normals keep their bits
    same = np.repeat(uv[:, :1], 3, axis=1)
    line = uv.copy()
    line[:, 2] = line[:, 0] + (line[:, 1] - line[:, 0]) * np.float32(2)
    counts = {}
    assert_bit_equal(trex.run(same, nmap64, counts=counts), trex.cam.normals_buffer, "three equal uv")
    assert counts["det_zero"] == 15801 and counts["written"] == 0
    out = trex.run(line, nmap64, counts=counts)
    assert counts["written"] + counts["det_zero"] == 15801 and counts["det_zero"] > 15000      # (rounding leaves a few dets)
    dead = trex.cam.normals_buffer.copy()
    dead[::2] = 0
    dead[1::4] = np.nan
    dead[3::8, :, 1] = np.inf
    out = trex.run(uv, nmap64, normals=dead, counts=counts)
    untouched = ~counts["mask"]
    assert untouched[::2].all() and untouched[1::4].all() and untouched[3::8].all() and counts["written"] > 1000
    assert_bit_equal(out[untouched], dead[untouched], "zero, NaN and infinite normals")
    assert not np.isnan(out[counts["mask"]]).any()
    # a negative strength is the opposite tilt of the same size
    a, b = trex.run(uv, nmap64, strength=0.5), trex.run(uv, nmap64, strength=-0.5)
    n = trex.cam.normals_buffer[trex.covered].astype(np.float64)
    nu = n / np.linalg.norm(n, axis=1, keepdims=True)
    ta, tb = (o[trex.covered] - (o[trex.covered].astype(np.float64) * nu).sum(1, keepdims=True) * nu for o in (a, b))
    assert np.abs(ta + tb).max() <= 1e-5


def test_a_bump_never_turns_a_normal_past_a_right_angle(trex, trex_uv, nmap64):
    """out . Nu == mz up to rounding.  Tu is Tp / |Tp| with Tp = Tt - Nu (Nu . Tt): its component along Nu is the
    rounding error of that difference, at most a few 2^-24 |Tt|, divided by |Tp|.  The bound below is 16 * 2^-24 *
    (1 + |Tt| / |Tp|) with the ratio recomputed here in float64."""
    uv = trex_uv[3]
    for filter in nmap_ref.FILTERS:
        out = trex.run(uv, nmap64, filter)
        ys, xs, t, s = nmap_ref.samples(trex.cam.winner, trex.tri, trex.cam.proj_mat, uv, nmap64, True, filter)
        mz = (s[:, 2].astype(np.float64) - 128.0) / 127.0
        n = trex.cam.normals_buffer[ys, xs].astype(np.float64)
        nu = n / np.linalg.norm(n, axis=1, keepdims=True)
        c, w = trex.tri[t].astype(np.float64), uv[t].astype(np.float64)
        e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        tt = e1 * (w[:, 2, 1] - w[:, 0, 1])[:, None] - e2 * (w[:, 1, 1] - w[:, 0, 1])[:, None]
        tp = tt - nu * (nu * tt).sum(1, keepdims=True)
        ratio = np.linalg.norm(tt, axis=1) / np.linalg.norm(tp, axis=1)
        err = np.abs((out[ys, xs].astype(np.float64) * nu).sum(1) - mz)
        print(f"{filter}: largest |out . Nu - mz| = {err.max():.3e}, largest |Tt| / |Tp| = {ratio.max():.3f}")
        assert (err <= 16 * 2.0 ** -24 * (1 + ratio)).all()
        assert mz.min() > 0.5 and ((out[ys, xs] * nu).sum(1) > 0).all()


@pytest.fixture(scope="module")
def quad(oracle):
    """A camera-facing square at z = 2, (u, v) = (0, 0), (1, 0), (1, 1), (0, 1) at its corners A, B, C, D: u along
    B - A and v along D - A, both along the screen's axes."""
    A, B, Cc, D = np.float32([[-0.6, -0.6, 2], [0.6, -0.6, 2], [0.6, 0.6, 2], [-0.6, 0.6, 2]])
    tri = np.ascontiguousarray(np.stack([np.stack([A, B, Cc]), np.stack([A, Cc, D])]), np.float32)
    uv = np.float32([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]])
    nrm = np.broadcast_to(np.float32([0, 0, -1]), (2, 3, 3)).copy()
    f = _Frame(oracle, (tri, np.full((2, 3, 3), 128.0, np.float32), nrm), 64, 64)
    f.uv, f.eu, f.ev = uv, (B - A).astype(np.float64), (D - A).astype(np.float64)
    assert f.covered.sum() > 1500 and set(np.unique(f.cam.winner)) == {-1, 0, 1}
    return f


def test_the_sign_convention_on_a_camera_facing_quad(quad):
    q = quad
    up_u = nmap_ref.from_height(np.tile((np.arange(32) * 8).astype(np.uint8), (32, 1)), 2.0)            # rises with u
    up_v = nmap_ref.from_height(np.tile((np.arange(32)[::-1] * 8).astype(np.uint8)[:, None], (1, 32)), 2.0)   # rises with v
    for filter in nmap_ref.FILTERS:
        for perspective in (False, True):
            counts = {}
            out = q.run(q.uv, up_u, filter, perspective, counts=counts)[q.covered].astype(np.float64)
            assert counts["written"] == counts["covered"] and counts["mirrored"] == 0
            assert (out @ q.eu < -0.05).all() and np.abs(out @ q.ev).max() <= 1e-6, (filter, perspective)
            assert (out[:, 2] < 0).all()                          # still towards the camera
            out = q.run(q.uv, up_v, filter, perspective)[q.covered].astype(np.float64)
            assert (out @ q.ev < -0.05).all() and np.abs(out @ q.eu).max() <= 1e-6, (filter, perspective)
    # u -> 1 - u: the surface direction of increasing u turns round, the texels' slope does not: the x tilt flips
    mirrored = q.uv.copy()
    mirrored[..., 0] = np.float32(1) - mirrored[..., 0]
    counts = {}
    out = q.run(mirrored, up_u, counts=counts)[q.covered].astype(np.float64)
    assert counts["mirrored"] == counts["covered"] == counts["written"]
    assert (out @ q.eu > 0.05).all() and np.abs(out @ q.ev).max() <= 1e-6
    out = q.run(mirrored, up_v)[q.covered].astype(np.float64)
    assert (out @ q.ev < -0.05).all()                              # v is as it was
    # normals that face away from the camera get the same tilt in the surface
    back = -q.cam.normals_buffer
    out = q.run(q.uv, up_u, normals=back)[q.covered].astype(np.float64)
    assert (out @ q.eu < -0.05).all() and (out[:, 2] > 0).all()


def test_swapping_two_corners_with_their_uv_changes_nothing_but_rounding(quad):
    """The same surface, the same mapping, the other winding: the frame comes from the uv, not from the corner order.
    The quad's triangles have 2 * area = 1.6e3 px^2 and coordinates below 64, so a barycentric is good to about
    64 * 64 * 2^-23 / 1.6e3 = 3e-7 and u, v alike; a 32-texel bilinear sample of bytes that step by at most 60 per texel
    then moves by at most 3e-7 * 32 * 60 / 127 = 5e-6 in the decoded vector, and the frame arithmetic adds a few 2^-24:
    the bound is 2e-5."""
    q = quad
    bumpy = nmap_ref.from_height(pass_scenes.texture(3, 32, 32)[:, :, 0] // 4, 1.0)
    a = q.run(q.uv, bumpy)
    for order in ([1, 0, 2], [0, 2, 1], [2, 1, 0]):
        swapped = _Frame.__new__(_Frame)
        swapped.tri, swapped.cam = np.ascontiguousarray(q.tri[:, order]), q.cam
        counts = {}
        b = swapped.run(np.ascontiguousarray(q.uv[:, order]), bumpy, counts=counts)
        # (an odd permutation of the corners turns the sign of det: every pixel counts as mirrored, and sg undoes it)
        assert counts["mirrored"] == counts["written"] == counts["covered"]
        diff = float(np.abs(a.astype(np.float64) - b).max())
        print(f"corners {order}: largest difference {diff:.3e}")
        assert diff <= 2e-5
    assert (np.abs(a - q.cam.normals_buffer)[q.covered].max(1) > 1e-3).all()       # and the map does tilt every normal


def test_a_row_strip_writes_only_its_rows(trex, trex_uv, nmap64):
    y0, y1 = 77, 163
    whole = trex.run(trex_uv[3], nmap64, "trilinear")
    counts = {}
    out = trex.run(trex_uv[3], nmap64, "trilinear", y0=y0, y1=y1, counts=counts)
    assert_bit_equal(out[:y0], trex.cam.normals_buffer[:y0], "rows above the strip")
    assert_bit_equal(out[y1:], trex.cam.normals_buffer[y1:], "rows below the strip")
    assert_bit_equal(out[y0:y1], whole[y0:y1], "the strip's rows")
    assert counts["covered"] == int(trex.covered[y0:y1].sum()) == counts["written"] > 1000
    assert not counts["mask"][:y0].any() and not counts["mask"][y1:].any()


def test_the_large_map_is_minified_and_the_chain_calms_it(trex, trex_uv):
    """Why the trilinear filter belongs to the pass: a 709 x 709 map on T-Rex at 256 x 256 is minified at every pixel."""
    uv = trex_uv[3]
    big = nmap_ref.from_height(pass_scenes.texture(8, 709, 709)[:, :, 0], 1.0)
    l0 = mip_ref.pixel_levels(trex.cam.winner, trex.tri, trex.cam.proj_mat, uv, 709, 709, True)[5]
    assert list(np.bincount(l0, minlength=10)) == [231, 9588, 5006, 808, 124, 32, 11, 0, 1, 0]
    n = trex.cam.normals_buffer[trex.covered].astype(np.float64)
    got = {}
    for filter in ("bilinear", "trilinear"):
        o = trex.run(uv, big, filter)[trex.covered].astype(np.float64)
        cs = (o * n).sum(1) / np.linalg.norm(o, axis=1) / np.linalg.norm(n, axis=1)
        ang = np.degrees(np.arccos(np.clip(cs, -1, 1)))
        got[filter] = (round(float(ang.mean()), 1), round(float(ang.max()), 1))
    assert got == {"bilinear": (17.9, 49.6), "trilinear": (3.7, 25.9)}


def test_the_counts_on_the_soup_with_random_uv(oracle, nmap64):
    tri, col, nrm, uv = pass_scenes.soup_textured(71, 3000, 256, size_px=(3.0, 50.0))
    f = _Frame(oracle, (tri, col, nrm), 256, 256)
    counts = {}
    f.run(uv, nmap64, counts=counts)
    counts.pop("mask")
    assert counts == dict(covered=65439, written=65439, det_zero=0, mirrored=33076, flipped=34174)


# ---- 5. float32 against float64 ----------------------------------------------------------------------------------------

# the measured maxima of the two soups (the docstring below)
SOUP_F64 = {71: {"nearest": 1.06e-5, "bilinear": 1.13e-5, "trilinear": 1.30e-6},
            72: {"nearest": 5.60e-6, "bilinear": 5.60e-6, "trilinear": 3.58e-6}}

def test_against_the_statements_in_float64(oracle, trex, trex_uv, nmap64):
    """The decode, the tangent frame and the result in float64 from the same float32 barycentrics, uv and samples.
    Measured, the largest componentwise difference of a written normal (components up to about 1.4): T-Rex 256^2
    3.81e-7 nearest, 1.75e-7 bilinear and trilinear; the soups of random normals and random uv, where a tangent can
    lie within a degree of the normal and |Tt| / |Tp| multiplies the rounding of Tp, 1.06e-5, 1.13e-5 and 1.30e-6
    (seed 71) and 5.60e-6, 5.60e-6 and 3.58e-6 (seed 72).  The assertion allows ten times the measured maximum of each frame.  It is a check of the model's
    statements, not a bound on the kernel, which is held to bit equality with the float32 model."""
    frames = [("trex", trex, trex_uv[3], {"nearest": 3.81e-7, "bilinear": 1.75e-7, "trilinear": 1.75e-7})]
    for seed, top in ((71, SOUP_F64[71]), (72, SOUP_F64[72])):
        tri, col, nrm, uv = pass_scenes.soup_textured(seed, 3000, 256, size_px=(3.0, 50.0))
        frames.append((f"soup{seed}", _Frame(oracle, (tri, col, nrm), 256, 256), uv, top))
    for name, f, uv, top in frames:
        for filter in nmap_ref.FILTERS:
            ca, cb = {}, {}
            a = f.run(uv, nmap64, filter, counts=ca)
            b = f.run(uv, nmap64, filter, counts=cb, dtype=np.float64)
            assert a.dtype == np.float32 and b.dtype == np.float64
            assert (ca["mask"] == cb["mask"]).all(), f"{name}, {filter}: a pixel changed its written / not-written decision"
            diff = float(np.abs(a.astype(np.float64) - b).max())
            print(f"{name}, {filter}: largest |float32 - float64| component difference: {diff:.3e}")
            assert 0 < diff <= 10 * top[filter], (name, filter)




# ---- the Renderer's checks, which need no GPU --------------------------------------------------------------------------

def test_renderer_refuses_what_cannot_work():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer

    class WithPass:
        bound = None

        def normal_map_pass(self):
            pass

        def bind_normal_map(self, normal_map=None, **kw):
            self.bound = (normal_map, kw)

        def get_normal_map(self):
            return None if self.bound is None else (self.bound[0] if self.bound[0] is not None else self.bound[1].get("height"))

    class Plain:
        pass
    flat = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="no normal_map_pass"):
        Renderer(Plain(), GuroIllumination(pass_scenes.LIGHT), normal_map=dict(normal_map=flat))
    with pytest.raises(ValueError, match="'fused'.*without a texture_pass"):
        Renderer(WithPass(), GuroIllumination(pass_scenes.LIGHT), on_device="fused", normal_map=dict(normal_map=flat))
    with pytest.raises(ValueError, match=r"\['uv_by_triangles'\] unknown"):
        Renderer(WithPass(), GuroIllumination(pass_scenes.LIGHT), normal_map=dict(normal_map=flat, uv_by_triangles=None))
    with pytest.raises(ValueError, match="needs 'normal_map' or 'height'"):
        Renderer(WithPass(), GuroIllumination(pass_scenes.LIGHT), normal_map=dict(strength=2.0))
    f = WithPass()
    r = Renderer(f, GuroIllumination(pass_scenes.LIGHT), on_device="fused", texture_pass={},
                 normal_map=dict(height=flat[..., 0], scale=3.0, filter="trilinear", strength=0.5))
    assert r.normal_map == dict(filter="trilinear", strength=0.5)
    assert f.bound[0] is None and sorted(f.bound[1]) == ["height", "mipmaps", "scale"]
    assert f.bound[1]["mipmaps"] is True and f.bound[1]["scale"] == 3.0 and f.bound[1]["height"] is not None
    for on_device in (None, False, True):
        assert Renderer(WithPass(), GuroIllumination(pass_scenes.LIGHT), on_device=on_device,
                        normal_map=dict(normal_map=flat)).normal_map == {}
    assert Renderer(Plain(), GuroIllumination(pass_scenes.LIGHT)).normal_map is None
