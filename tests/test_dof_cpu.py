"""Depth of field without a GPU: the header against the binding and the library, the unit's place in the build tables,
the entry point's argument checks, the host model the GPU tests compare with (tests/dof_ref.py) pinned by identities on
the oracle's T-Rex frame and on a two-plane scene whose radii are known, and against its own float64 evaluation;
``AdvancedPixelBufferFiller.depth_of_field``'s protocol on CPU tensors, ``Renderer(depth_of_field=...)`` and
``depth_of_field.view_depth``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dof_ref
from pass_scenes import Frame, capi, fake_filler_base, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from util import assert_bit_equal, other_symbols, own_unit_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crender_dof_blur"
_vp, _i32, _f = C.c_void_p, C.c_int, C.c_float
DOF_ARGTYPES = [_vp, _vp, _vp, C.c_int64, _vp, C.POINTER(C.c_float), _vp, _f, _f, _f, _i32, _vp, _i32, _i32, _i32, _i32,
                C.c_uint, _vp]


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_dof_symbol_is_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_dof.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["dof"]) == {ENTRY}
    assert not declared & other_symbols(capi, "dof")
    res, args = capi.UNIT_SIGNATURES["dof"][ENTRY]
    assert res == C.c_int and args == DOF_ARGTYPES == getattr(capi.load(), ENTRY).argtypes
    decl = re.search(r"CRENDER_API int " + ENTRY + r"\((.*?)\);", header, re.S).group(1)
    params = [" ".join(a.split()) for a in decl.split(",")]
    assert params == ["const int32_t *d_winner", "const float *d_z", "const float *d_tri", "int64_t T", "const uint32_t *d_pos_of",
                      "const float *P16", "const float *d_color", "float focus", "float band", "float aperture",
                      "int max_radius", "float *d_out", "int H", "int W", "int y0", "int y1", "unsigned flags", "void *stream"]
    assert len(params) == len(args) == 18
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert ENTRY in set(re.findall(r" T (crender_\w+)", out))
    top = int(re.search(r"#define CRENDER_DOF_MAX_RADIUS (\d+)", header).group(1))
    assert top == capi.DOF_MAX_RADIUS == dof_ref.MAX_RADIUS == 12
    # five planes of the largest staged tile and what follows them stay below 64 KB: no launch attribute
    assert 5 * (32 + 2 * top) ** 2 * 4 == 62720 and 62720 + (4 + 13 * 13) * 4 < 65536
    assert capi.ABI_VERSION == 6


def test_dof_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit = new = own_unit_source(_build, "dof", "dof.hip", "crender_dof.h")
    head = "// ---- depth of field (crender_dof_blur) ----"
    assert unit.count(head) == 1
    assert unit.index(head) < unit.index("void k_dof_blur") < unit.index("int crender_dof_blur(")
    # a unit of its own: its namespace and its entry points, the passes' frame from the shared header as it is
    assert new.count("namespace {") == 1 and new.count('extern "C" {') == 1
    for name in ("tile_lane(", "tile_origin(", "tile_grid(", "tile_lds_bytes(", "frame_checks(", "rows_check(", "arg_error(",
                 "wave_any(", "wave_reduce<true>("):
        assert name in new and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    assert "CR_DEV" not in new and "asm" not in new
    # one staging barrier and one at the end of a tile; no tap divides or takes a root
    body = new[new.index("void k_dof_blur"):new.index("}  // namespace")]
    assert "extern __shared__" in body and body.count("__syncthreads()") == 2
    taps = body[body.index("for (int dy = -Rt"):body.index("if (!inside) continue;")]
    code = "".join(line.split("//")[0] for line in taps.splitlines())
    assert "/" not in code and "sqrtf" not in code and "wave_any(take[0]" in code
    shape = new.index("projection_shape_check(E, P16)")          # winner_pass.h's, shared with ao.hip and motion.hip
    assert new.index("frame_checks(E") < new.index("rows_check(E") < shape < new.index("focus is not")


def test_dof_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    P = capi.f32_16(np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]]))
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)      # never dereferenced: every call below fails its checks first
    nan, inf = float("nan"), float("inf")

    def blur(win=fake, z=fake, tri=fake, T=4, pos_of=None, P=P, col=fake, focus=1.0, band=0.0, aperture=4.0, R=8, out=other,
             H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_dof_blur(win, z, tri, T, pos_of, P, col, focus, band, aperture, R, out, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(win=None), dict(z=None), dict(P=None), dict(col=None), dict(out=None)):
        assert blur(**kw) == E and "d_winner, d_z, P16, d_color or d_out is NULL" in text(), kw
    for bad in (-1, -2 ** 40):
        assert blur(T=bad) == E and "T is negative" in text()
    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert blur(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert blur(**kw) == E and "rows outside the frame" in text(), kw
    for flags in (1, 2, 0x80000000):
        assert blur(flags=flags) == E and "unknown flag bits" in text(), flags
    assert blur(out=fake) == E and "d_out is d_color" in text()
    # the projection's shape, in the occlusion pass's words
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
    for bad in (0.0, -1.0, nan, inf, -inf):
        assert blur(focus=bad) == E and "focus is not finite and positive" in text(), bad
    for bad in (-1e-9, nan, inf):
        assert blur(band=bad) == E and "band is not finite and 0 or above" in text(), bad
        assert blur(aperture=bad) == E and "aperture is not finite and 0 or above" in text(), bad
    for bad in (0, -1, 13, 2 ** 31 - 1, -2 ** 31):
        assert blur(R=bad) == E and "max_radius is not 1 .. 12" in text(), bad
    assert text().startswith("crender_dof_blur: ")
    # the order: the frame, the rows, the flags, the planes, the projection, then focus, band, aperture, max_radius
    Q = (C.c_float * 16)(*P)
    Q[1] = 1.0
    assert blur(T=-1, H=0, y0=9, flags=1, out=fake, P=Q, focus=0.0) == E and "T is negative" in text()
    assert blur(H=0, y0=9, flags=1, out=fake, P=Q, focus=0.0) == E and "H or W is below 1" in text()
    assert blur(y0=9, flags=1, out=fake, P=Q, focus=0.0) == E and "rows outside the frame" in text()
    assert blur(flags=1, out=fake, P=Q, focus=0.0) == E and "unknown flag bits" in text()
    assert blur(out=fake, P=Q, focus=0.0) == E and "d_out is d_color" in text()
    assert blur(P=Q, focus=0.0) == E and "an entry that must be 0" in text()
    assert blur(focus=0.0, band=-1.0, aperture=-1.0, R=0) == E and "focus" in text()
    assert blur(band=-1.0, aperture=-1.0, R=0) == E and "band" in text()
    assert blur(aperture=-1.0, R=0) == E and "aperture" in text()
    # d_tri and d_pos_of are never read: NULL with T > 0 is no error.  Such a call goes on to its launch; it is made here
    # only where no device could run it, and ends in the runtime's refusal, never in EINVAL.
    if not torch.cuda.is_available():
        assert blur(tri=None) in (capi.OK, capi.EHIP)
        assert blur(T=0, tri=None, aperture=0.0, band=0.0, R=12, H=1, W=1, y1=1) in (capi.OK, capi.EHIP)


# ---- the model on a two-plane scene ------------------------------------------------------------------------------

HB = WB = 64
PROJ = np.float32([[2.4, 0, 0, 0], [0, 2.4, 0, 0], [0, 0, 1.0002, 1.0], [0, 0, -0.2, 0]])      # a matrix of the shape
NEAR_C, FAR_C = np.float32([200.0, 100.0, 50.0]), np.float32([40.0, 80.0, 160.0])


def _z_of(zv):
    """A z-plane value whose view depth is near zv (the model rebuilds it by its own statement)."""
    return np.float32(PROJ[2, 2]) + np.float32(PROJ[3, 2]) / np.float32(zv)


def _two_planes(near=1.0, far=4.0, box=(24, 40)):
    """(winner, z, colour): triangle 1 far behind the whole frame, triangle 0 near on the square box x box."""
    winner = np.ones((HB, WB), np.int32)
    z = np.full((HB, WB), _z_of(far), np.float32)
    color = np.empty((HB, WB, 3), np.float32)
    color[:] = FAR_C
    sel = (slice(*box), slice(*box))
    winner[sel], z[sel], color[sel] = 0, _z_of(near), NEAR_C
    return winner, z, color


def _blur(winner, z, color, **kw):
    kw.setdefault("T", 2)
    return dof_ref.dof_blur(color, winner, z, kw.pop("T"), PROJ, **kw)


def test_a_sharp_foreground_against_a_blurred_background():
    winner, z, color = _two_planes()
    near = float(dof_ref.view_depth(PROJ, _z_of(1.0)))
    c = {}
    out = _blur(winner, z, color, focus=near, aperture=8.0, max_radius=8, counts=c)
    s, ia = dof_ref.coc(winner, z, 2, PROJ, near, 0.0, 8.0, 8)
    assert (s[winner == 0] == 0).all() and (ia[winner == 0] == 1).all()
    far_s = np.unique(s[winner == 1])
    assert len(far_s) == 1 and 5.9 < far_s[0] < 6.1 and c["largest_c"] == float(far_s[0])      # 8 * (4 - 1) / 4
    # the foreground keeps its bits right up to its edge: the background behind it does not bleed over it
    assert_bit_equal(out[winner == 0], color[winner == 0], "the foreground")
    assert c["copied"] == 16 * 16 and c["blurred"] == HB * WB - 16 * 16 and c["covered"] == HB * WB
    # and what is in front spreads by ITS radius, which is 0: the background beside the square takes nothing of it, and
    # being of one colour stays that colour within the rounding of a sum of n <= 17^2 products and one of as many weights
    assert np.abs(out[winner == 1] - FAR_C).max() <= 255 * (17 * 17 + 1) * 2.0 ** -23
    assert (out[winner == 1].view(np.uint32) != np.tile(FAR_C, (int((winner == 1).sum()), 1)).view(np.uint32)).any()


def test_a_blurred_foreground_spreads_over_what_is_in_focus():
    winner, z, color = _two_planes()
    far = float(dof_ref.view_depth(PROJ, _z_of(4.0)))
    out = _blur(winner, z, color, focus=far, aperture=2.0, max_radius=12)
    s = dof_ref.coc(winner, z, 2, PROJ, far, 0.0, 2.0, 12)[0]
    near_s = np.unique(s[winner == 0])
    assert (s[winner == 1] == 0).all() and len(near_s) == 1 and -6.1 < near_s[0] < -5.9       # 2 * (1 - 4) / 1
    # the distance of every pixel to the square: within r + 1 = 7 of it the in-focus background changes, at 7 and
    # beyond (k <= 0) it keeps its bits
    ax = np.arange(HB)
    off = np.maximum(np.maximum(24 - ax, ax - 39), 0)
    dist = np.hypot(off[:, None], off[None, :])
    changed = (out.view(np.uint32) != color.view(np.uint32)).any(2)
    ring, away = (dist > 0) & (dist < 7), dist >= 7
    assert changed[ring].all() and ring.sum() > 500
    # the square itself sums over its own pixels only (a sharp background spreads by ITS radius, 0): its colour, rounded
    assert np.abs(out[winner == 0] - NEAR_C).max() <= 255 * (13 * 13 + 1) * 2.0 ** -23
    assert not changed[away].any() and away.sum() > 2000
    # the clamp: the same at max_radius 3, where the square reaches 3 + 1 px
    out3 = _blur(winner, z, color, focus=far, aperture=2.0, max_radius=3)
    changed3 = (out3.view(np.uint32) != color.view(np.uint32)).any(2)
    assert changed3[32, 40:43].all() and not changed3[32, 44:].any()


def test_special_values_and_what_is_copied():
    winner, z, color = _two_planes()
    near = float(dof_ref.view_depth(PROJ, _z_of(1.0)))
    color[30, 30] = np.float32([-0.0, np.nan, np.inf])
    color[31, 31].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]     # NaN payloads and -0
    # aperture = 0 copies everything, bit for bit, whatever z holds
    odd = z.copy()
    odd[5, 5:10] = [np.nan, np.inf, -np.inf, PROJ[2, 2], 1e6]
    assert_bit_equal(_blur(winner, odd, color, focus=near, aperture=0.0, max_radius=12), color, "aperture = 0")
    # in focus, the planted colours are copied with their bits
    out = _blur(winner, z, color, focus=near, aperture=8.0, max_radius=8)
    assert_bit_equal(out[24:40, 24:40], color[24:40, 24:40], "the foreground with a -0 and NaNs")
    # the odd depths: a NaN z and the division by zero give s = NaN, which contributes nowhere; +-inf clamp to +-Rf
    s = dof_ref.coc(winner, odd, 2, PROJ, near, 0.0, 8.0, 8)[0]
    assert np.isnan(s[5, 5]) and np.isnan(s[5, 8]) and s[5, 6] == 8 and s[5, 7] == -8
    # winners that name no triangle are background: s = aperture, clamped
    w2 = winner.copy()
    w2[0, :4] = [-2, 2, 2 ** 31 - 1, -2 ** 31]
    assert (dof_ref.coc(w2, z, 2, PROJ, near, 0.0, 5.0, 8)[0][0, :4] == 5).all()
    assert (dof_ref.coc(w2, z, 2, PROJ, near, 0.0, 50.0, 8)[0][0, :4] == 8).all()
    assert (dof_ref.coc(winner, z, 0, PROJ, near, 0.0, 3.0, 8)[0] == 3).all()              # T = 0
    # a band: the far plane within it is sharp as well, and then nothing is blurred at all
    c = {}
    assert_bit_equal(_blur(winner, z, color, focus=near, aperture=8.0, band=3.5, counts=c), color, "a band over both planes")
    assert c["blurred"] == 0 and c["largest_c"] == 0
    # a strip: rows outside are `out`'s, and are not seen
    sentinel = np.full_like(color, -7.0)
    strip = _blur(winner, z, color, focus=near, aperture=8.0, y0=20, y1=50, out=sentinel)
    assert (strip[:20] == -7).all() and (strip[50:] == -7).all()
    poisoned_c, poisoned_w, poisoned_z = color.copy(), winner.copy(), z.copy()
    poisoned_c[:20], poisoned_c[50:], poisoned_w[:20], poisoned_z[50:] = 1e9, np.nan, 0, np.nan
    assert_bit_equal(_blur(poisoned_w, poisoned_z, poisoned_c, focus=near, aperture=8.0, y0=20, y1=50, out=sentinel), strip,
                     "rows outside the strip are not read")
    whole = _blur(winner, z, color, focus=near, aperture=8.0)
    assert_bit_equal(whole[28:42], strip[28:42], "rows out of the edge's reach")
    assert (whole[20] != strip[20]).any()


def test_the_pruned_window_is_the_full_window():
    """Offsets beyond ceil(the largest c) are never taken: the model with and without them, radii below the clamp."""
    winner, z, color = _two_planes(far=1.6)
    rng = np.random.default_rng(3)
    color = rng.uniform(0, 255, color.shape).astype(np.float32)
    near = float(dof_ref.view_depth(PROJ, _z_of(1.0)))
    for aperture in (6.0, 2.5):
        a, b = {}, {}
        full = _blur(winner, z, color, focus=near, aperture=aperture, max_radius=12, prune=False, counts=a)
        assert_bit_equal(_blur(winner, z, color, focus=near, aperture=aperture, max_radius=12, counts=b), full, "pruned")
        assert a == b and 0 < a["largest_c"] < 3 and a["blurred"] > 1000


# ---- identities on the oracle's frames -------------------------------------------------------------------------

class _Frame(Frame):
    def run(self, focus=None, **kw):
        T = len(self.tri)
        focus = self.median if focus is None else focus
        return dof_ref.dof_blur(kw.pop("color", self.cam.color_buffer), self.cam.winner, self.cam.z_buffer, T, self.cam.proj_mat,
                                focus, **kw)

    @property
    def median(self):
        return float(np.median(dof_ref.view_depth(self.cam.proj_mat, self.cam.z_buffer)[self.covered]))


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_wire_pass_cpu.py's scenes

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


def test_identities_on_trex(trex):
    f = trex
    base = f.cam.color_buffer
    zv = dof_ref.view_depth(f.cam.proj_mat, f.cam.z_buffer)
    # aperture = 0 copies, -0 and NaN colours included
    odd = base.copy()
    odd[f.covered] = np.where(np.random.default_rng(1).uniform(size=(int(f.covered.sum()), 3)) < 0.1, np.float32(np.nan), odd[f.covered])
    odd[~f.covered] = np.float32(-0.0)
    for R in (1, 12):
        assert_bit_equal(f.run(aperture=0.0, max_radius=R, color=odd), odd, f"aperture = 0, max_radius {R}")
    # a band around the median depth: the pixels in it that no blurred pixel reaches are copied, the others are not
    band = 0.06
    c = {}
    out = f.run(aperture=16.0, band=band, max_radius=8, counts=c)
    print(f"T-Rex 256^2, aperture 16, band {band}, max_radius 8: {c}")
    assert c["covered"] == 15801 and c["copied"] + c["blurred"] == 256 * 256
    assert c["copied"] >= 0.05 * 256 * 256 and c["blurred"] >= 0.05 * 256 * 256
    changed = (out.view(np.uint32) != base.view(np.uint32)).any(2)
    s = dof_ref.coc(f.cam.winner, f.cam.z_buffer, len(f.tri), f.cam.proj_mat, f.median, band, 16.0, 8)[0]
    assert (np.abs(zv - np.float32(f.median))[f.covered & (s == 0)] <= np.float32(band)).all()
    assert (s[~f.covered] == 8).all()                    # the background, clamped
    assert (changed & (s != 0)).sum() > 5000 and (changed & (s == 0)).sum() > 100       # blurred, and reached by a blurred one
    assert not changed[~f.covered].all()                # (the cleared background is one colour, 0, and stays it)
    assert not np.isnan(out).any()
    # every output channel lies within what the window holds
    lo, hi = base.min(), base.max()
    assert out.min() >= lo - 1e-3 and out.max() <= hi + 1e-3
    # one colour everywhere stays that colour within the rounding of n <= 17^2 products, their sum and the weights' sum
    flat = np.broadcast_to(np.float32([173.25, 21.5, 250.125]), base.shape)
    got = f.run(aperture=16.0, band=band, max_radius=8, color=np.ascontiguousarray(flat))
    assert np.abs(got - flat).max() <= 255 * (17 * 17 + 1) * 2.0 ** -23
    assert (got.view(np.uint32) != np.ascontiguousarray(flat).view(np.uint32)).any()


F64_MEASURED = 5.112e-4              # measured with this model: 2.059e-4 on T-Rex, 3.148e-4 on seed 51, 5.112e-4 on seed 71


def test_float32_against_float64(trex, soups):
    """The same statements in float64 from the same float32 planes, every pixel of the three frames, aperture 16, a band
    of 0.06 and max_radius 8; colours are 0 .. 255.  A pixel is a quotient of two sums of up to 17^2 positive terms, each
    term a product with a weight that is itself a difference of nearby numbers ((r + 1) - dist): the sums' roundings of
    2^-24 each on values up to 255 times the weights, and the cancellation in k.  No pixel of these frames takes another
    tap set in float64 that weighs visibly.  The bound is ten times the largest measured difference: the margin is for
    frames not measured.  A check of the model's statements, not a bound on the kernel, which is held to bit equality with
    the float32 model."""
    worst = 0.0
    for name, f in (("trex", trex), ("soup51", soups[51]), ("soup71", soups[71])):
        kw = dict(aperture=16.0, band=0.06, max_radius=8)
        o32 = f.run(**kw)
        o64 = f.run(dtype=np.float64, **kw)
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and not np.isnan(o64).any()
        diff = float(np.abs(o32.astype(np.float64) - o64).max())
        print(f"{name}: largest |out - out64| = {diff:.3e}")
        worst = max(worst, diff)
    print(f"largest |out - out64| over the three frames = {worst:.3e} (bound {10 * F64_MEASURED:.3e})")
    assert 0 < worst <= 10 * F64_MEASURED


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._deferred_passes import DeferredPasses  # noqa: E402


class FakeFiller(fake_filler_base()):
    """The protocol of the two mixins on CPU tensors; the launch is the host model."""

    def _launch_pass(self, entry, args):
        winner, z, tri, T, pos_of, P, color, focus, band, aperture, R, out, h, w, y0, y1, flags = args
        self.events.append((entry, T, focus, band, aperture, R, flags))
        assert color is self.color_buffer and out is not color and (h, w, y0, y1) == (self.h, self.w, self.y0, self.y1)
        assert all(type(v) is float for v in (focus, band, aperture)) and type(R) is int
        got = dof_ref.dof_blur(color.numpy(), winner.numpy(), z.numpy(), T, P, focus, aperture=aperture, band=band, max_radius=R,
                               y0=y0, y1=y1, out=out.numpy())
        out.copy_(torch.from_numpy(got))


def test_depth_of_field_returns_a_new_tensor_and_leaves_the_views_as_they_were(soups):
    s = soups[71]
    T = len(s.tri)
    f = FakeFiller(s)
    kw = dict(aperture=6.0, band=0.05, max_radius=4)
    out = f.depth_of_field(s.median, **kw)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (s.H, s.W, 3)
    assert f.events == ["push", "settle", ("crender_dof_blur", T, s.median, 0.05, 6.0, 4, 0)]     # edits, the settle, the launch
    want = s.run(**kw)
    assert (want != s.cam.color_buffer).any()
    assert_bit_equal(out.numpy(), want, "the model's plane")
    assert not f._host_fresh and not f._host_exposed                     # nobody asked for a view: as stale as before
    assert_bit_equal(f.color_buffer.numpy(), s.cam.color_buffer, "the colour plane is only read")
    # the defaults
    f.depth_of_field(np.float32(1.5))
    assert f.events[-1] == ("crender_dof_blur", T, 1.5, 0.0, 4.0, 8, 0)
    sig = inspect.signature(DeferredPasses.depth_of_field)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == \
        [("focus", inspect.Parameter.empty), ("aperture", 4.0), ("band", 0.0), ("max_radius", 8)]
    # an edit made in a view is carried up first and blurred; the views stay fresh
    view = f.get_color_buffer()
    assert f._host_fresh and f._host_exposed
    view[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    f.events.clear()
    again = f.depth_of_field(s.median, **kw)
    assert again is not out and f._host_fresh and not f._host_exposed and f.events[0] == "push"
    edited = s.cam.color_buffer.copy()
    edited[100:140, 100:140] = np.float32([10.0, 100.0, 200.0])
    assert_bit_equal(again.numpy(), s.run(color=edited, **kw), "over the edited colours")
    assert f.get_color_buffer() is view
    # a row strip fills its rows and leaves the others zero
    g = FakeFiller(s, row_strip=(37, 75))
    strip = g.depth_of_field(s.median, **kw).numpy()
    assert not strip[:37].any() and not strip[75:].any()
    assert_bit_equal(strip[37:75], s.run(y0=37, y1=75, **kw)[37:75], "the strip's rows")


def test_depth_of_field_refuses_what_edge_aa_refuses_and_names_bad_arguments(soups):
    s = soups[71]
    f = FakeFiller(s)
    f._pipeline = object()
    with pytest.raises(ValueError, match=r"depth_of_field is not available on a swap chain \(pipeline=True\)"):
        f.depth_of_field(1.0)
    with pytest.raises(ValueError, match="depth_of_field needs the winner plane"):
        FakeFiller(s, track_winner=False).depth_of_field(1.0)
    f = FakeFiller(s)
    f._inputs = None
    with pytest.raises(ValueError, match="depth_of_field: no frame has been rendered"):
        f.depth_of_field(1.0)
    f = FakeFiller(s)
    f._last_flags = 0
    with pytest.raises(ValueError, match="depth_of_field: the last frame did not start from cleared buffers"):
        f.depth_of_field(1.0)
    f = FakeFiller(s)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e39, True, "1", None):
        with pytest.raises(ValueError, match="focus must be a finite view depth above 0, got " + re.escape(repr(bad))):
            f.depth_of_field(bad)
    for name in ("aperture", "band"):
        for bad in (-1.0, float("nan"), float("inf"), False, "2", None):
            with pytest.raises(ValueError, match=name + " must be a finite number, 0 or above, got " + re.escape(repr(bad))):
                f.depth_of_field(1.0, **{name: bad})
    for bad in (0, 13, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="max_radius must be an int from 1 to 12, got " + re.escape(repr(bad))):
            f.depth_of_field(1.0, max_radius=bad)
    assert f.events == []                                                 # nothing was pushed, settled or launched
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    assert AdvancedPixelBufferFiller.depth_of_field is DeferredPasses.depth_of_field


# ---- the Renderer ----------------------------------------------------------------------------------------------

# a filler that records what the Renderer asks of it; ``image`` is what its pass returns
IMAGE = torch.arange(8 * 8 * 3, dtype=torch.float32).reshape(8, 8, 3)
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass phong_pass ao_pass shade_guro bind_environment environment_pass get_color_tensor "
    "get_color_buffer depth_of_field",
    returns=dict(depth_of_field=IMAGE), quiet="_push_host_edits synchronize get_normals_buffer", image=IMAGE)


def test_renderer_construction():
    from cython3dmodelrenderer_amd.renderer import Renderer
    params = inspect.signature(Renderer.__init__).parameters
    assert "depth_of_field" in params and params["depth_of_field"].default is None
    assert Renderer(SimpleNamespace(), None).depth_of_field is None

    class Plain:
        pass

    class Lens:
        def depth_of_field(self, focus, aperture=4.0, band=0.0, max_radius=8):
            pass

        def edge_aa(self, edges=None):
            pass

        def resolve(self, s):
            pass
    with pytest.raises(ValueError, match=r"Renderer\(depth_of_field=\.\.\.\) needs a filler with a depth-of-field pass.*Plain has no depth_of_field"):
        Renderer(Plain(), None, depth_of_field=dict(focus=1.0))
    with pytest.raises(ValueError, match="depth_of_field.*antialias.*supersample"):
        Renderer(Lens(), None, depth_of_field=dict(focus=1.0), antialias={})
    with pytest.raises(ValueError, match="depth_of_field.*antialias.*supersample"):
        Renderer(Lens(), None, depth_of_field=dict(focus=1.0), supersample=2)
    with pytest.raises(ValueError, match=r"\['radius'\] unknown"):
        Renderer(Lens(), None, depth_of_field=dict(focus=1.0, radius=2))
    with pytest.raises(ValueError, match="needs 'focus'"):
        Renderer(Lens(), None, depth_of_field={})
    opts = dict(focus=1.25, aperture=6.0, band=0.1, max_radius=12)
    r = Renderer(Lens(), None, depth_of_field=opts)
    assert r.depth_of_field == opts and r.depth_of_field is not opts
    assert Renderer(Lens(), None, antialias={}).depth_of_field is None


def test_renderer_runs_the_pass_last_and_returns_its_plane():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    model = SimpleNamespace(_vertices_by_triangles=np.zeros((1, 3, 3), np.float32))
    guro = GuroIllumination((0.3, -0.2, 1.0))
    opts = dict(focus=1.25, aperture=6.0)
    # fused: a cleared frame, the pass last, its tensor handed out
    f = _Recorder()
    r = Renderer(f, guro, on_device="fused", depth_of_field=opts)
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "get_color_tensor", "depth_of_field"]
    assert f.calls[1][2].get("clear") is True and f.calls[-1] == ("depth_of_field", (), opts)
    # on the device, after the light and after the wire pass, every frame
    f = _Recorder()
    r = Renderer(f, guro, on_device=True, wireframe=dict(width=2.0), depth_of_field=opts)
    assert r.render(model) is f.image and r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "shade_guro", "wire_pass", "get_color_tensor",
                                       "depth_of_field"] * 2
    assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    # None and False return a fresh numpy copy of the pass's plane
    for on_device in (None, False):
        f = _Recorder()
        got = Renderer(f, guro, on_device=on_device, depth_of_field=opts).render(model)
        assert isinstance(got, np.ndarray) and np.array_equal(got, f.image.numpy())
        assert f.calls[-1] == ("depth_of_field", (), opts) and [c[0] for c in f.calls].count("depth_of_field") == 1
        assert all(c[2].get("clear") is True for c in f.calls if c[0] == "render_model")
    # a PhongIllumination with ambient occlusion and lines: ao, light, lines, and the pass after them all
    f = _Recorder()
    r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), on_device=True, ambient_occlusion={}, wireframe={}, depth_of_field=opts)
    assert r.render(model) is f.image
    assert [c[0] for c in f.calls] == ["set_fused_illumination", "render_model", "ao_pass", "phong_pass", "wire_pass",
                                       "get_color_tensor", "depth_of_field"]
    # without the option nothing changes: no pass, the filler's own colours
    f = _Recorder()
    assert Renderer(f, guro, on_device="fused").render(model) == "colour"
    assert "depth_of_field" not in [c[0] for c in f.calls] and f.calls[1][2] == dict(clear=True)


# ---- view_depth ------------------------------------------------------------------------------------------------

def test_view_depth_is_the_kernels_statement(trex):
    from cython3dmodelrenderer_amd import _capi, depth_of_field
    P, z = trex.cam.proj_mat, trex.cam.z_buffer
    want = dof_ref.view_depth(P, z)
    got = depth_of_field.view_depth(P, z)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert_bit_equal(got, want, "a plane")
    assert_bit_equal(depth_of_field.view_depth(_capi.f32_16(P), z), want, "the filler's 16 floats")
    assert_bit_equal(depth_of_field.view_depth(P, torch.from_numpy(z)).numpy(), want, "a tensor")
    y, x = np.argwhere(trex.covered)[1000]
    one = depth_of_field.view_depth(P, z[y, x])
    assert one.dtype == np.float32 and one == want[y, x] and 0.5 < float(one) < 2.0
    assert depth_of_field.view_depth(P, float(z[y, x])) == want[y, x]
    # the depth a pixel shows, focused on: that pixel's circle of confusion is 0
    s = dof_ref.coc(trex.cam.winner, z, len(trex.tri), P, float(one), 0.0, 8.0, 8)[0]
    assert s[y, x] == 0 and (s[trex.covered] != 0).sum() > 10000
    # the division by zero and a NaN do not raise
    odd = depth_of_field.view_depth(P, np.float32([P[2, 2], np.nan]))
    assert np.isinf(odd[0]) and np.isnan(odd[1])
