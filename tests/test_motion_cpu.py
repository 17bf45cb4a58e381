"""Motion vectors and motion blur without a GPU: the header against the binding and the library, the unit's place in the
build, the entry points' argument checks, the host model the GPU tests
compare with (tests/motion_ref.py) pinned by hand-made scenes, against its own float64 evaluation and against the oracle's
frame of the previous pose; ``AdvancedPixelBufferFiller.motion_vectors`` / ``motion_blur``'s protocol on CPU tensors and
``Renderer(motion_blur=...)``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import motion_ref
from pass_scenes import Frame, capi, fake_filler_base, oracle_frame, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import assert_bit_equal, other_symbols, own_unit_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS, BLUR = "crender_motion_vectors", "crender_motion_blur"
_vp, _i32, _f = C.c_void_p, C.c_int, C.c_float
_f32p = C.POINTER(C.c_float)
VECTORS_ARGTYPES = [_vp, _vp, C.c_int64, _vp, _f32p, _vp, _f, _vp, _i32, _i32, _i32, _i32, C.c_uint, _vp]
BLUR_ARGTYPES = [_vp, _vp, _vp, C.c_int64, _vp, _f32p, _vp, _vp, _i32, _i32, _f, _vp, _i32, _i32, _i32, _i32, C.c_uint, _vp]


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_motion_symbols_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_motion.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["motion"]) == {VECTORS, BLUR}
    assert not declared & other_symbols(capi, "motion")
    L = capi.load()
    for name, want in ((VECTORS, VECTORS_ARGTYPES), (BLUR, BLUR_ARGTYPES)):
        res, args = capi.UNIT_SIGNATURES["motion"][name]
        assert res == C.c_int and args == want == getattr(L, name).argtypes, name
    decl = {n: [" ".join(a.split()) for a in re.search(r"CRENDER_API int " + n + r"\((.*?)\);", header, re.S).group(1).split(",")]
            for n in (VECTORS, BLUR)}
    assert decl[VECTORS] == ["const int32_t *d_winner", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                             "const float *P16", "const float *d_prev_tri", "float exposure", "float *d_velocity", "int H",
                             "int W", "int y0", "int y1", "unsigned flags", "void *stream"]
    assert decl[BLUR] == ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T",
                          "const uint32_t *d_pos_of", "const float *P16", "const float *d_color", "const float *d_velocity",
                          "int max_radius", "int taps", "float soft", "float *d_out", "int H", "int W", "int y0", "int y1",
                          "unsigned flags", "void *stream"]
    assert len(decl[VECTORS]) == len(VECTORS_ARGTYPES) == 14 and len(decl[BLUR]) == len(BLUR_ARGTYPES) == 18
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert {VECTORS, BLUR} <= set(re.findall(r" T (crender_\w+)", out))
    top = int(re.search(r"#define CRENDER_MOTION_MAX_RADIUS (\d+)", header).group(1))
    taps = int(re.search(r"#define CRENDER_MOTION_MAX_TAPS (\d+)", header).group(1))
    assert top == capi.MOTION_MAX_RADIUS == motion_ref.MAX_RADIUS == 12
    assert taps == capi.MOTION_MAX_TAPS == motion_ref.MAX_TAPS == 32
    far = np.float32(float(re.search(r"#define CRENDER_MOTION_FAR (\S+)f", header).group(1)))
    assert far == motion_ref.FAR == np.finfo(np.float32).max
    # five planes of the largest staged tile and what follows them stay below 64 KB: no launch attribute
    assert 5 * (32 + 2 * top) ** 2 * 4 == 62720 and 62720 + (2 * 4 + 2 * taps) * 4 < 65536
    assert capi.ABI_VERSION == 6                                  # the change is additive


def test_motion_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    # the unit's place in the build, and the four includes of a pass, in dof.hip's order
    text = own_unit_source(_build, "motion", "motion.hip", "crender_motion.h")
    assert text.count("namespace {") == 1 and text.count('extern "C" {') == 1 and "asm" not in text
    assert text.index("void k_motion_vectors") < text.index("void k_motion_blur") < text.index("int crender_motion_vectors(")
    # the blur: one staging barrier, one behind the tap table and one at the end of a tile; no tap divides or takes a root
    body = text[text.index("void k_motion_blur"):text.index("}  // namespace")]
    assert "extern __shared__" in body and body.count("__syncthreads()") == 3
    taps = body[body.index("for (int i0 = 0"):body.index("if (!inside) continue;")]
    code = "".join(line.split("//")[0] for line in taps.splitlines())
    assert "/" not in code and "sqrtf" not in code and "wave_any(take[0]" in code
    # the host checks R, N and the LDS size before the launch
    entry = text[text.index("int crender_motion_blur("):]
    assert entry.index("max_radius is not") < entry.index("taps is not") < entry.index("lds > 65536") < entry.index("hipLaunchKernelGGL")


def _matrix(capi):
    return capi.f32_16(np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]]))


def test_motion_vectors_argument_errors_without_a_gpu(capi):
    L, E = capi.load(), capi.EINVAL
    P = _matrix(capi)
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)        # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")

    def vec(win=fake, tri=fake, T=4, pos_of=None, P=P, prev=fake, exposure=1.0, out=other, H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_motion_vectors(win, tri, T, pos_of, P, prev, exposure, out, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(P=None), dict(out=None)):
        assert vec(**kw) == E and "d_winner, P16 or d_velocity is NULL" in text(), kw
    for bad in (-1, -2 ** 40):
        assert vec(T=bad) == E and "T is negative" in text()
    for kw in (dict(tri=None), dict(prev=None)):
        assert vec(**kw) == E and "d_tri or d_prev_tri is NULL with T > 0" in text(), kw
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert vec(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert vec(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (1, 2, 0x80000000):
        assert vec(flags=flags) == E and "unknown flag bits" in text(), flags
    for bad in (-1e-9, -1.0, nan, inf, -inf):
        assert vec(exposure=bad) == E and "exposure is not finite and 0 or above" in text(), bad
    assert text().startswith("crender_motion_vectors: ")
    # the order
    assert vec(win=None, T=-1, H=0, y0=9, flags=1, exposure=nan) == E and "is NULL" in text()
    assert vec(T=-1, H=0, y0=9, flags=1, exposure=nan) == E and "T is negative" in text()
    assert vec(tri=None, H=0, y0=9, flags=1, exposure=nan) == E and "with T > 0" in text()
    assert vec(H=0, y0=9, flags=1, exposure=nan) == E and "H or W is below 1" in text()
    assert vec(y0=9, flags=1, exposure=nan) == E and "rows outside the frame" in text()
    assert vec(flags=1, exposure=nan) == E and "unknown flag bits" in text()


def test_motion_blur_argument_errors_without_a_gpu(capi):
    L, E = capi.load(), capi.EINVAL
    P = _matrix(capi)
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)
    nan, inf = float("nan"), float("inf")

    def blur(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, col=fake, vel=fake, R=8, N=16, soft=0.02, out=other, H=8, W=8,
             y0=0, y1=8, flags=0):
        return L.crender_motion_blur(win, z, tri, T, pos_of, P, col, vel, R, N, soft, out, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(z=None), dict(P=None), dict(col=None), dict(vel=None), dict(out=None)):
        assert blur(**kw) == E and "d_winner, d_z, P16, d_color, d_velocity or d_out is NULL" in text(), kw
    for bad in (-1, -2 ** 40):
        assert blur(T=bad) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert blur(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert blur(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (1, 2, 0x80000000):
        assert blur(flags=flags) == E and "unknown flag bits" in text(), flags
    assert blur(out=fake) == E and "d_out is d_color" in text()
    for i in (1, 2, 4, 6, 8, 9, 12, 13):
        Q = (C.c_float * 16)(*P)
        Q[i] = 0.5
        assert blur(P=Q) == E and "P16 is not of crender_projection_matrix's shape (an entry that must be 0 is not)" in text(), i
        Q[i] = nan
        assert blur(P=Q) == E and "an entry that must be 0 is not" in text(), i
    for i in (0, 5, 14):
        for bad in (0.0, nan, inf):
            Q = (C.c_float * 16)(*P)
            Q[i] = bad
            assert blur(P=Q) == E and "entry 0, 5 or 14 is 0 or not finite" in text(), (i, bad)
    for bad in (0, -1, 13, 2 ** 31 - 1, -2 ** 31):
        assert blur(R=bad) == E and "max_radius is not 1 .. 12" in text(), bad
    for bad in (0, -1, 33, 2 ** 31 - 1, -2 ** 31):
        assert blur(N=bad) == E and "taps is not 1 .. 32" in text(), bad
    for bad in (0.0, -0.02, nan, inf, -inf):
        assert blur(soft=bad) == E and "soft is not finite and positive" in text(), bad
    assert text().startswith("crender_motion_blur: ")
    # the order: the frame, the rows, the flags, the planes, the projection, then max_radius, taps, soft
    Q = (C.c_float * 16)(*P)
    Q[1] = 1.0
    assert blur(T=-1, H=0, y0=9, flags=1, out=fake, P=Q, R=0) == E and "T is negative" in text()
    assert blur(H=0, y0=9, flags=1, out=fake, P=Q, R=0) == E and "H or W is below 1" in text()
    assert blur(y0=9, flags=1, out=fake, P=Q, R=0) == E and "rows outside the frame" in text()
    assert blur(flags=1, out=fake, P=Q, R=0) == E and "unknown flag bits" in text()
    assert blur(out=fake, P=Q, R=0) == E and "d_out is d_color" in text()
    assert blur(P=Q, R=0) == E and "an entry that must be 0" in text()
    assert blur(R=0, N=0, soft=0.0) == E and "max_radius" in text()
    assert blur(N=0, soft=0.0) == E and "taps" in text()
    # d_tri and d_pos_of are never read: NULL with T > 0 is no error.  Such a call goes on to its launch; it is made here
    # only where no device could run it, and ends in the runtime's refusal, never in EINVAL.
    if not torch.cuda.is_available():
        assert blur(tri=None) in (capi.OK, capi.EHIP)


# ---- the model on hand-made scenes -----------------------------------------------------------------------------

HB = WB = 96
PROJ = np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]])      # a matrix of the shape
NEAR, FAR = 1.0, 4.0
BOX = (slice(32, 64), slice(32, 64))


def _z_of(zv):
    """A z-plane value whose view depth is near zv (the model rebuilds it by its own statement)."""
    return np.float32(PROJ[2, 2]) + np.float32(PROJ[3, 2]) / np.float32(zv)


def _occluder(v_near, v_far, seed=1):
    """(winner, z, colour, velocity): triangle 1 far behind the whole frame moving by v_far, triangle 0 near on the square
    32 .. 63 (a whole tile) moving by v_near; random colours."""
    winner = np.ones((HB, WB), np.int32)
    z = np.full((HB, WB), _z_of(FAR), np.float32)
    color = np.random.default_rng(seed).uniform(0, 255, (HB, WB, 3)).astype(np.float32)
    vel = np.empty((HB, WB, 2), np.float32)
    vel[:] = np.float32(v_far)
    winner[BOX], z[BOX], vel[BOX] = 0, _z_of(NEAR), np.float32(v_near)
    return winner, z, color, vel


def _blur(winner, z, color, vel, **kw):
    return motion_ref.motion_blur(color, winner, z, kw.pop("T", 2), PROJ, vel, **kw)


def _changed(out, color):
    return (out.view(np.uint32) != color.view(np.uint32)).any(2)


def test_a_quad_translated_in_x_has_the_analytic_velocity(oracle):
    """A fronto-parallel quad at depth 2 whose previous pose lies dx to the left: every pixel of it moved by
    dx * P00 / depth * W / 2 pixels in x and not at all in y.  Measured against the float64 evaluation of the same
    statements the float32 velocity differs by at most 7.7e-6 pixels here; ten times that is allowed (the margin is for
    other hosts' libm-free arithmetic being the same: there is none to speak of)."""
    H = W = 128
    depth, dx = np.float32(2.0), np.float32(0.05)
    a = np.float32(0.5)
    quad = np.float32([[[-a, -a, depth], [a, -a, depth], [a, a, depth]], [[-a, -a, depth], [a, a, depth], [-a, a, depth]]])
    nrm = np.zeros((2, 3, 3), np.float32)
    nrm[..., 2] = -1
    cam = oracle_frame(oracle, quad, np.full((2, 3, 3), 100, np.float32), nrm, H, W)
    covered = cam.winner >= 0
    assert 3000 < covered.sum() < 8000
    prev = quad.copy()
    prev[..., 0] -= dx
    v = motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, prev)
    v64 = motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, prev, dtype=np.float64)
    want = float(dx) * float(cam.proj_mat[0, 0]) / float(depth) * W / 2
    assert 3.5 < want < 4.5
    worst = float(np.abs(v.astype(np.float64) - v64).max())
    print(f"a translated quad: analytic vx {want:.6f}, largest |v - v64| = {worst:.3e}")
    assert 0 < worst <= 10 * 7.7e-6
    assert np.abs(v64[covered][:, 0] - want).max() < 1e-6 and np.abs(v64[covered][:, 1]).max() < 1e-6
    assert np.abs(v[covered][:, 0] - want).max() <= 10 * 7.7e-6 + 1e-6 and np.abs(v[covered][:, 1]).max() <= 10 * 7.7e-6
    assert not v[~covered].any() and not np.signbit(v[~covered]).any()          # the background: +0
    # the exposure scales it; 0 leaves zeros
    half = motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, prev, exposure=0.5)
    assert_bit_equal(half, v * np.float32(0.5), "exposure 0.5")
    assert not motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, prev, exposure=0.0).any()
    # a previous pose behind the camera, and one that projects to infinity: no velocity
    behind = quad.copy()
    behind[..., 2] = -1
    assert not motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, behind).any()
    huge = quad.copy()
    huge[..., 0] = 3e38
    huge[..., 2] = 1e-38
    assert not motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, huge).any()
    # a strip writes its rows and leaves the others as they were
    sentinel = np.full((H, W, 2), -7, np.float32)
    strip = motion_ref.motion_vectors(cam.winner, quad, cam.proj_mat, prev, y0=40, y1=70, out=sentinel)
    assert (strip[:40] == -7).all() and (strip[70:] == -7).all()
    assert_bit_equal(strip[40:70], v[40:70], "the strip's rows")


def test_what_copies():
    winner, z, color, vel = _occluder((0, 0), (0, 0))
    color[40, 40].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]     # NaN payloads and -0
    color[10, 10] = np.float32([np.inf, -np.inf, np.nan])
    c = {}
    assert_bit_equal(_blur(winner, z, color, vel, counts=c), color, "a zero velocity plane")
    assert c["tiles_copied"] == 9 and c["copied"] == HB * WB and c["blurred"] == c["taps_taken"] == c["moving"] == 0
    # taps = 1: the one offset is (0, 0)
    winner, z, _, vel = _occluder((9, -5), (-3, 14))
    c = {}
    assert_bit_equal(_blur(winner, z, color, vel, taps=1, counts=c), color, "taps = 1")
    assert c["tiles_copied"] == 0 and c["moving"] == HB * WB and c["copied"] == HB * WB
    # a velocity of exactly one pixel is a half length of exactly 1/2: the tile copies; the next float does not
    for v1, copies in ((np.float32(1.0), True), (np.nextafter(np.float32(1.0), np.float32(2.0)), False)):
        vel = np.zeros((HB, WB, 2), np.float32)
        vel[..., 0] = v1
        c = {}
        _blur(winner, z, color, vel, taps=32, max_radius=4, counts=c)
        assert (c["tiles_copied"] == 9) == copies and (c["moving"] == 0) == copies
    # non-finite velocities count as none; a huge finite one clamps to max_radius with D = 0: no offset, a copy
    vel = np.zeros((HB, WB, 2), np.float32)
    vel[5, 5], vel[6, 6], vel[7, 7], vel[50, 50] = (np.nan, 3), (np.inf, 0), (2, -np.inf), (1e30, 1e30)
    c = {}
    assert_bit_equal(_blur(winner, z, color, vel, counts=c), color, "odd velocities")
    hx, hy, l = motion_ref.half_velocity(vel, 8)
    assert l[5, 5] == l[6, 6] == l[7, 7] == 0 and l[50, 50] == 8 and hx[50, 50] == hy[50, 50] == 0
    assert c["largest_l"] == 8 and c["moving"] == 1 and c["tiles_copied"] == 8 and c["copied"] == HB * WB


def test_a_flat_frame_changes_by_rounding_only():
    winner, z, _, vel = _occluder((13, 6), (-4, 9))
    flat = np.ascontiguousarray(np.broadcast_to(np.float32([173.25, 21.5, 250.125]), (HB, WB, 3)))
    c = {}
    out = _blur(winner, z, flat, vel, taps=32, max_radius=12, counts=c)
    assert c["blurred"] > 0.9 * HB * WB
    # the quotient of a sum of n <= 33 products by the sum of their weights
    assert np.abs(out - flat).max() <= 255 * (33 + 1) * 2.0 ** -23
    assert _changed(out, flat).any()


def test_a_static_occluder_over_a_moving_floor_keeps_its_bits():
    for R, v in ((8, (16, 0)), (12, (-30, 30)), (4, (3, -7))):
        winner, z, color, vel = _occluder((0, 0), v)
        c = {}
        out = _blur(winner, z, color, vel, max_radius=R, taps=32, counts=c)
        ch = _changed(out, color)
        assert_bit_equal(out[BOX], color[BOX], f"the occluder, floor moving by {v}")
        assert ch[winner == 1].mean() > 0.95 and c["tiles_copied"] == 0 and c["moving"] == HB * WB - 32 * 32
        # and with the depths the other way round the moving surface is in FRONT: it spreads over the static square
        z2 = np.where(winner == 0, _z_of(FAR), _z_of(NEAR)).astype(np.float32)
        assert _changed(_blur(winner, z2, color, vel, max_radius=R, taps=32), color)[BOX].any()


def test_a_moving_occluder_reaches_just_short_of_max_radius_into_a_static_floor():
    """The square moves in x by more than 2 R, so its half length clamps to l = R exactly and every tile that sees it
    within its halo walks D = (R, 0).  A floor pixel at distance d of the square takes a tap of it iff cone(d / l) > 0,
    d < R: the smear is R - 1 columns on both sides, in the square's rows only, and not one further (the contract's
    "up to max_radius and no further": the cone is 0 AT R, and the static floor's own cylinder is 0 from d = 1 on).
    32 taps of D = (R, 0) hit every integer offset up to R."""
    for R in (2, 4, 8, 12):
        winner, z, color, vel = _occluder((2 * R + 3, 0), (0, 0))
        out = _blur(winner, z, color, vel, max_radius=R, taps=32)
        ch = _changed(out, color)
        assert ch[BOX].all()
        assert not ch[:32].any() and not ch[64:].any()                       # the motion is along x
        assert ch[32:64, 32 - (R - 1):32].all() and ch[32:64, 64:64 + (R - 1)].all()
        assert not ch[:, :32 - (R - 1)].any() and not ch[:, 64 + (R - 1):].any()
        # moving in y instead: the same in the columns
        winner, z, color, vel = _occluder((0, -(2 * R + 3)), (0, 0))
        ch = _changed(_blur(winner, z, color, vel, max_radius=R, taps=32), color)
        assert ch[32 - (R - 1):32, 32:64].all() and not ch[:32 - (R - 1)].any() and not ch[64 + (R - 1):].any()
        assert not ch[:, :32].any() and not ch[:, 64:].any()


def test_the_dominant_pixel_and_the_taps():
    # the taps of D = (8, 0) with 16 taps: tau = +-15/16 gives 7.5, which rint takes to 8; 13/16 gives 6.5, to 6
    ox, oy, dist = motion_ref.tile_taps(np.float32(8), np.float32(0), 16, 8)
    assert ox.tolist() == [-8, -6, -6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6, 8] and not oy.any()
    assert dist.dtype == np.float32 and dist.tolist() == np.abs(ox).astype(np.float32).tolist()
    ox, oy, dist = motion_ref.tile_taps(np.float32(-3), np.float32(4), 2, 12)          # tau = -+1/2: -1.5 -> -2, 2 -> 2
    assert ox.tolist() == [2, -2] and oy.tolist() == [-2, 2] and dist.tolist() == [np.sqrt(np.float32(8))] * 2
    # two pixels of equal largest l: the first in frame order is the dominant one of every tile that stages both
    winner, z, color, vel = _occluder((0, 0), (0, 0))
    vel[40, 50], vel[40, 45], vel[39, 60] = (0, 10), (10, 0), (6, 8)
    dom = []
    _blur(winner, z, color, vel, max_radius=8, dominant=dom)
    assert len(dom) == 9 and dom[4] == (32, 32, 60, 39)
    vel[39, 60] = 0
    dom = []
    _blur(winner, z, color, vel, max_radius=8, dominant=dom)
    assert dom[4] == (32, 32, 45, 40)
    # a dominant pixel in the halo's corner: pixel (31, 31) is in the halo of the centre tile at max_radius 1 and above
    vel[:] = 0
    vel[31, 31] = (5, 5)
    for R, seen in ((1, {0, 1, 3, 4}), (8, {0, 1, 3, 4})):
        dom = []
        c = {}
        _blur(winner, z, color, vel, max_radius=R, dominant=dom, counts=c)
        assert {i for i, d in enumerate(dom) if d[2:] == (31, 31)} == seen and c["tiles_copied"] == 5
    vel[31, 31] = 0
    vel[23, 23] = (5, 5)                                                    # 9 pixels before the centre tile: out of its halo
    dom = []
    _blur(winner, z, color, vel, max_radius=8, dominant=dom)
    assert [i for i, d in enumerate(dom) if d[2:] == (23, 23)] == [0]


# ---- the model on the oracle's frames --------------------------------------------------------------------------

class _Frame(Frame):
    def previous(self, angles):
        return motion_ref.rotated(self.tri, angles)

    def vectors(self, prev, **kw):
        return motion_ref.motion_vectors(self.cam.winner, self.tri, self.cam.proj_mat, prev, **kw)

    def run(self, velocity, **kw):
        return motion_ref.motion_blur(kw.pop("color", self.cam.color_buffer), self.cam.winner, self.cam.z_buffer, len(self.tri),
                                      self.cam.proj_mat, velocity, **kw)


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_wire_pass_cpu.py's scenes

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


def test_the_static_pose_copies(trex, soups):
    """The previous pose is the current one: the blend of a triangle's own corners with its own barycentrics gives the
    pixel back up to rounding (at most 3.1e-5 of a pixel on T-Rex, 5.54e-5 on the soups), far below the half pixel."""
    for name, f, top in (("trex", trex, 3.2e-5), ("soup51", soups[51], 5.6e-5), ("soup71", soups[71], 5.6e-5)):
        v = f.vectors(f.tri)
        worst = float(np.abs(v).max())
        print(f"{name}: largest static |v| = {worst:.3e}")
        assert 0 < worst <= top
        odd = f.cam.color_buffer.copy()
        odd[~f.covered] = np.float32(-0.0)
        for R in (1, 12):
            c = {}
            assert_bit_equal(f.run(v, max_radius=R, taps=32, color=odd, counts=c), odd, f"{name}: a static pose, max_radius {R}")
            assert c["moving"] == 0 and c["tiles_copied"] * 1024 >= f.H * f.W


V64_MEASURED = 6.144e-5      # measured with this model: 6.143e-5 on T-Rex (10 deg y), 5.293e-5 on seed 51, 5.211e-5 on seed 71 (5 deg z)
C64_MEASURED = 4.406e-4      # colours, max_radius 8, 16 taps: 5.362e-5 on T-Rex, 4.405e-4 on seed 51, 4.200e-4 on seed 71


def test_float32_against_float64(trex, soups):
    """The same statements in float64 from the same float32 inputs.  The velocity is a projected blend: a handful of
    roundings of 2^-24 on screen coordinates up to 256.  The colour is a quotient of two sums of up to 17 terms on values
    up to 255; the float64 blur walks the float32 velocity plane, so both evaluations take the same dominant pixels (a
    dominant half velocity that rounds another way at an rint tie would move a tap by a pixel: it does on seed 71 rotated
    by 3 degrees about y, where half of the pixels are clamped to max_radius and D * tau sits on halves — there one pixel
    differs by 82, a step of the rule and not a rounding, so that pose is not measured here).  The bounds are ten times
    the largest measured difference: the margin is for frames not measured.  A check of the model's statements, not a
    bound on the kernels, which are held to bit equality with the float32 model."""
    worst_v = worst_c = 0.0
    for name, f, angles in (("trex", trex, (0, 10, 0)), ("soup51", soups[51], (0, 0, 5)), ("soup71", soups[71], (0, 0, 5))):
        prev = f.previous(angles)
        v32, v64 = f.vectors(prev), f.vectors(prev, dtype=np.float64)
        assert v32.dtype == np.float32 and v64.dtype == np.float64 and np.isfinite(v32).all() and np.isfinite(v64).all()
        dv = float(np.abs(v32.astype(np.float64) - v64).max())
        o32 = f.run(v32, max_radius=8, taps=16)
        o64 = f.run(v32, max_radius=8, taps=16, dtype=np.float64)
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and not np.isnan(o64).any()
        dc = float(np.abs(o32.astype(np.float64) - o64).max())
        print(f"{name}: largest |v - v64| = {dv:.3e}, largest |out - out64| = {dc:.3e}")
        worst_v, worst_c = max(worst_v, dv), max(worst_c, dc)
    print(f"largest over the frames: velocity {worst_v:.3e} (bound {10 * V64_MEASURED:.3e}), colour {worst_c:.3e} "
          f"(bound {10 * C64_MEASURED:.3e})")
    assert 0 < worst_v <= 10 * V64_MEASURED and 0 < worst_c <= 10 * C64_MEASURED


# (covered pixels whose previous position is on the frame, of those the ones whose triangle won there in the oracle's
# frame of the previous pose), and the model's counts at max_radius 8, 16 taps
CONSISTENT = {
    ("trex", (0, 10, 0)): (15801, 11813, 14364, 29, 52090, 13446, 91593),        # 0.748
    ("trex", (0, 2, 0)): (15801, 12607, 5753, 31, 62790, 2746, 25050),           # 0.798
    ("soup71", (0, 0, 5)): (62822, 58160, 65037, 0, 2126, 63410, 672301),        # 0.926
    ("soup71", (0, 3, 0)): (60410, 37909, 63733, 0, 466, 65070, 769879),         # 0.628
}


@pytest.mark.parametrize("scene,angles", list(CONSISTENT))
def test_the_vectors_lead_to_the_same_triangle_in_the_previous_frame(oracle, trex, soups, scene, angles):
    """Where a pixel's surface point was, the rasterizer of the PREVIOUS pose mostly drew the same triangle: on the oracle's
    frame of the previous pose, the winner at the rounded previous position is the pixel's own triangle for more than half
    of the covered pixels (not all: the point may have been hidden, or a neighbour won the rounded pixel)."""
    f = trex if scene == "trex" else soups[71]
    prev = f.previous(angles)
    before = oracle_frame(oracle, prev, f.col, f.nrm, f.H, f.W)
    v = f.vectors(prev)
    ys, xs = np.nonzero(f.covered)
    px = np.rint(xs - v[ys, xs, 0].astype(np.float64)).astype(np.int64)
    py = np.rint(ys - v[ys, xs, 1].astype(np.float64)).astype(np.int64)
    on = (px >= 0) & (px < f.W) & (py >= 0) & (py < f.H)
    same = before.winner[py[on], px[on]] == f.cam.winner[ys[on], xs[on]]
    c = {}
    f.run(v, max_radius=8, taps=16, counts=c)
    got = (int(on.sum()), int(same.sum()), c["moving"], c["tiles_copied"], c["copied"], c["blurred"], c["taps_taken"])
    print(f"{scene} {angles}: {same.mean():.3f} of {on.sum()} lead to the same triangle; {c}")
    assert same.sum() > 0.5 * f.covered.sum()
    assert got == CONSISTENT[scene, angles]
    assert c["copied"] + c["blurred"] == f.H * f.W and c["covered"] == f.covered.sum()


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launch is the host model."""

    def _launch_pass(self, entry, args):
        if entry == VECTORS:
            winner, tri, T, pos_of, P, prev, exposure, out, h, w, y0, y1, flags = args
            self.events.append((entry, T, exposure, flags))
            assert type(exposure) is float and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
            got = motion_ref.motion_vectors(winner.numpy(), tri.numpy(), P, prev.numpy(), exposure, y0, y1, out=out.numpy())
        else:
            winner, z, tri, T, pos_of, P, color, vel, R, N, soft, out, h, w, y0, y1, flags = args
            self.events.append((entry, T, R, N, soft, flags))
            assert color is self.color_buffer and out is not color and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
            assert type(R) is int and type(N) is int and type(soft) is float
            got = motion_ref.motion_blur(color.numpy(), winner.numpy(), z.numpy(), T, P, vel.numpy(), R, N, soft, y0, y1,
                                         out=out.numpy())
        out.copy_(torch.from_numpy(got))


def test_the_two_methods_return_new_tensors_and_leave_the_views_as_they_were(soups):
    s = soups[71]
    T = len(s.tri)
    prev = s.previous((0, 0, 5))
    f = FakeFiller(s)
    v = f.motion_vectors(prev, exposure=0.75)
    assert isinstance(v, torch.Tensor) and v.dtype == torch.float32 and tuple(v.shape) == (s.H, s.W, 2)
    assert f.events == ["push", "settle", (VECTORS, T, 0.75, 0)]
    assert_bit_equal(v.numpy(), s.vectors(prev, exposure=0.75), "the model's vectors")
    kw = dict(max_radius=6, taps=9, soft=0.05)
    f.events.clear()
    out = f.motion_blur(prev, exposure=0.75, **kw)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (s.H, s.W, 3)
    assert f.events == ["push", "settle", (VECTORS, T, 0.75, 0), "push", "settle", (BLUR, T, 6, 9, 0.05, 0)]
    want = s.run(v.numpy(), **kw)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(out.numpy(), want, "the model's plane")
    assert not f._host_fresh and not f._host_exposed                     # nobody asked for a view: as stale as before
    assert_bit_equal(f.color_buffer.numpy(), s.cam.color_buffer, "the colour plane is only read")
    # velocity= of motion_vectors' own result is the same image; numpy goes as well
    f.events.clear()
    assert_bit_equal(f.motion_blur(velocity=v, **kw).numpy(), want, "velocity=, a tensor")
    assert f.events == ["push", "settle", (BLUR, T, 6, 9, 0.05, 0)]
    assert_bit_equal(f.motion_blur(velocity=v.numpy(), **kw).numpy(), want, "velocity=, numpy")
    assert_bit_equal(f.motion_blur(torch.from_numpy(prev), exposure=0.75, **kw).numpy(), want, "previous_vertices, a tensor")
    # the defaults
    f.motion_blur(prev)
    assert f.events[-1] == (BLUR, T, 8, 16, 0.02, 0) and f.events[-4] == (VECTORS, T, 1.0, 0)
    sig = inspect.signature(DeferredPasses.motion_blur)
    assert [(p.name, p.default, p.kind == p.KEYWORD_ONLY) for p in sig.parameters.values()][1:] == \
        [("previous_vertices", None, False), ("velocity", None, True), ("exposure", 1.0, True), ("max_radius", 8, True),
         ("taps", 16, True), ("soft", 0.02, True)]
    sig = inspect.signature(DeferredPasses.motion_vectors)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [("previous_vertices", inspect.Parameter.empty), ("exposure", 1.0)]
    # an edit made in a view is carried up first and blurred; the views stay fresh
    view = f.get_color_buffer()
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    f.events.clear()
    again = f.motion_blur(velocity=v, **kw)
    assert again is not out and f._host_fresh and not f._host_exposed and f.events[0] == "push"
    edited = s.cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    assert_bit_equal(again.numpy(), s.run(v.numpy(), color=edited, **kw), "over the edited colours")
    assert f.get_color_buffer() is view
    # a row strip fills its rows and leaves the others zero, in both planes
    g = FakeFiller(s, row_strip=(37, 75))
    vs = g.motion_vectors(prev).numpy()
    assert not vs[:37].any() and not vs[75:].any() and vs[37:75].any()
    strip = g.motion_blur(prev, **kw).numpy()
    assert not strip[:37].any() and not strip[75:].any()
    assert_bit_equal(strip[37:75], s.run(s.vectors(prev, y0=37, y1=75), y0=37, y1=75, **kw)[37:75], "the strip's rows")


def test_the_two_methods_refuse_what_depth_of_field_refuses_and_name_bad_arguments(soups):
    s = soups[71]
    prev = s.previous((0, 0, 5))
    for name, call in (("motion_vectors", lambda f: f.motion_vectors(prev)), ("motion_blur", lambda f: f.motion_blur(prev))):
        f = FakeFiller(s)
        f._pipeline = object()
        with pytest.raises(ValueError, match=name + r" is not available on a swap chain \(pipeline=True\)"):
            call(f)
        with pytest.raises(ValueError, match=name + " needs the winner plane"):
            call(FakeFiller(s, track_winner=False))
        f = FakeFiller(s)
        f._inputs = None
        with pytest.raises(ValueError, match=name + ": no frame has been rendered"):
            call(f)
        f = FakeFiller(s)
        f._last_flags = 0
        with pytest.raises(ValueError, match=name + ": the last frame did not start from cleared buffers"):
            call(f)
    f = FakeFiller(s)
    T = len(s.tri)
    for name, call in (("motion_vectors", f.motion_vectors), ("motion_blur", f.motion_blur)):
        with pytest.raises(ValueError, match=f"{name}: previous_vertices holds {T - 1} triangles, the last frame drew {T}"):
            call(prev[1:])
        with pytest.raises(ValueError, match=r"previous_vertices must have shape \[T, 3, 3\]"):
            call(prev.reshape(-1, 3))
        with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'float' but got 'double'"):
            call(prev.astype(np.float64))
        for bad in (-1.0, float("nan"), float("inf"), 1e39, True, "1", None):
            with pytest.raises(ValueError, match="exposure must be a finite number, 0 or above, got " + re.escape(repr(bad))):
                call(prev, exposure=bad)
    with pytest.raises(ValueError, match="motion_vectors: previous_vertices is None"):
        f.motion_vectors(None)
    v = np.zeros((s.H, s.W, 2), np.float32)
    with pytest.raises(ValueError, match="exactly one of previous_vertices and velocity"):
        f.motion_blur()
    with pytest.raises(ValueError, match="exactly one of previous_vertices and velocity"):
        f.motion_blur(prev, velocity=v)
    with pytest.raises(ValueError, match=r"exposure=0.5 with velocity="):
        f.motion_blur(velocity=v, exposure=0.5)
    for bad in (v[1:], v[..., :1], v.astype(np.float64), np.zeros((s.H, s.W, 3), np.float32)):
        with pytest.raises(ValueError, match=rf"velocity must be float32 \[{s.H}, {s.W}, 2\], the frame's, got"):
            f.motion_blur(velocity=bad)
    for bad in (0, 13, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="max_radius must be an int from 1 to 12, got " + re.escape(repr(bad))):
            f.motion_blur(prev, max_radius=bad)
    for bad in (0, 33, -1, 16.0, True, None):
        with pytest.raises(ValueError, match="taps must be an int from 1 to 32, got " + re.escape(repr(bad))):
            f.motion_blur(prev, taps=bad)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50, True, "1", None):
        with pytest.raises(ValueError, match="soft must be a finite range of view depths above 0, got " + re.escape(repr(bad))):
            f.motion_blur(prev, soft=bad)
    assert f.events == []                                                 # nothing was pushed, settled or launched
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.motion_blur is DeferredPasses.motion_blur
    assert AdvancedPixelBufferFiller.motion_vectors is DeferredPasses.motion_vectors


# ---- the Renderer ----------------------------------------------------------------------------------------------

# a filler that records what the Renderer asks of it (the pose as it was at the call: the model moves in place); ``image`` is
# what its pass returns
IMAGE = torch.arange(8 * 8 * 3, dtype=torch.float32).reshape(8, 8, 3)
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass phong_pass shade_guro bloom get_color_tensor get_color_buffer motion_blur",
    returns=dict(bloom="bloomed", motion_blur=IMAGE), quiet="_push_host_edits synchronize get_normals_buffer",
    copies=("motion_blur",), image=IMAGE)


def test_renderer_construction():
    from cython3dmodelrenderer_amd.renderer import Renderer
    names = list(inspect.signature(Renderer.__init__).parameters)
    at = names.index("motion_blur")
    assert names[at - 1] == "depth_of_field" and names[at + 1:] == ["normal_map", "environment", "bloom", "transparency",
                                                                      "wireframe", "supersample"]
    assert inspect.signature(Renderer.__init__).parameters["motion_blur"].default is None
    assert Renderer(SimpleNamespace(), None).motion_blur is None

    class Plain:
        pass

    class Shutter:
        def motion_blur(self, previous_vertices=None, **kw):
            pass

        depth_of_field = edge_aa = resolve = transparency_pass = motion_blur
    with pytest.raises(ValueError, match=r"Renderer\(motion_blur=\.\.\.\) needs a filler with a motion-blur pass.*Plain has no motion_blur"):
        Renderer(Plain(), None, motion_blur={})
    for other in (dict(antialias={}), dict(depth_of_field=dict(focus=1.0)), dict(supersample=2), dict(transparency=dict(alpha=0.5))):
        with pytest.raises(ValueError, match="motion_blur.*antialias.*depth_of_field.*supersample.*transparency"):
            Renderer(Shutter(), None, motion_blur={}, **other)
    with pytest.raises(ValueError, match=r"\['shutter'\] unknown"):
        Renderer(Shutter(), None, motion_blur=dict(shutter=2))
    opts = dict(exposure=0.5, max_radius=12, taps=32, soft=0.1)
    r = Renderer(Shutter(), None, motion_blur=opts)
    assert r.motion_blur == opts and r.motion_blur is not opts
    assert Renderer(Shutter(), None, motion_blur={}).motion_blur == {}


def test_renderer_keeps_the_pose_of_the_call_before_and_runs_the_pass_last():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    pose0 = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    model = SimpleNamespace(_vertices_by_triangles=pose0.copy())
    guro = GuroIllumination((0.3, -0.2, 1.0))
    opts = dict(exposure=0.5, taps=8)
    f = _Recorder()
    r = Renderer(f, guro, on_device="fused", motion_blur=opts)
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "get_color_tensor", "motion_blur"]
    assert f.calls[1][2].get("clear") is True and f.calls[-1][2] == opts
    assert np.array_equal(f.calls[-1][1][0].numpy(), pose0)                 # the first call: the pose itself, a copy
    # the model moves IN PLACE: the second call gets the copy kept from the first
    model._vertices_by_triangles += 1
    assert r.render(model) is f.image
    assert np.array_equal(f.calls[-1][1][0].numpy(), pose0)
    model._vertices_by_triangles += 1
    r.render(model)
    assert np.array_equal(f.calls[-1][1][0].numpy(), pose0 + 1)
    # reset_motion: the current pose again
    r.reset_motion()
    r.render(model)
    assert np.array_equal(f.calls[-1][1][0].numpy(), pose0 + 2)
    # another triangle count: the current pose
    model._vertices_by_triangles = np.zeros((5, 3, 3), np.float32)
    r.render(model)
    assert tuple(f.calls[-1][1][0].shape) == (5, 3, 3)
    # a tensor model
    model._vertices_by_triangles = torch.ones((5, 3, 3))
    r.render(model)
    assert not f.calls[-1][1][0].any()
    model._vertices_by_triangles += 1
    r.render(model)
    assert (f.calls[-1][1][0] == 1).all()
    # on the device after the light and the wire pass; None and False return a fresh numpy copy
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0), motion_blur=opts)
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "shade_guro", "wire_pass", "get_color_tensor",
                                       "motion_blur"]
    for on_device in (None, False):
        f = _Recorder()
        got = Renderer(f, guro, on_device=on_device, motion_blur={}).render(model)
        assert isinstance(got, np.ndarray) and np.array_equal(got, f.image.numpy())
        assert [c[0] for c in f.calls].count("motion_blur") == 1 and f.calls[-1][0] == "motion_blur"
        assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    # a PhongIllumination, and bloom after the pass, over its tensor
    f = _Recorder()
    r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), on_device=True, motion_blur={}, bloom={})
    assert r.render(model) == "bloomed"
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "phong_pass", "get_color_tensor", "motion_blur",
                                       "bloom"]
    assert f.calls[-1][2]["source"] is f.image
    # without the option nothing changes
    f = _Recorder()
    assert Renderer(f, guro, on_device="fused").render(model) == "colour"
    assert "motion_blur" not in [c[0] for c in f.calls] and f.calls[1][2] == dict(clear=True)
