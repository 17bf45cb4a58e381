"""The supersampling resolve without a GPU: the header against the binding and the build lists, the entry point's
argument checks, the host model the GPU tests compare with (tests/ssaa_ref.py) pinned by hand, and the protocol of
``DevicePlanes.resolve`` on CPU tensors (a subclass whose ``_resolve_planes`` calls the model, as
tests/test_host_views_cpu.py runs the rest of that class)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import ssaa_ref
from pass_scenes import capi  # noqa: F401 (fixtures)
from util import INCLUDE, assert_bit_equal, other_symbols, unit_in_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_ssaa_header_symbol_is_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_ssaa.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["ssaa"]) == {"crender_ssaa_resolve"}
    assert not declared & other_symbols(capi, "ssaa")
    L = capi.load()
    assert L.crender_ssaa_resolve.argtypes == capi.UNIT_SIGNATURES["ssaa"]["crender_ssaa_resolve"][1]
    # argument counts: the declaration's commas against the table
    decl = re.search(r"CRENDER_API int crender_ssaa_resolve\((.*?)\);", header, re.S).group(1)
    res, args = capi.UNIT_SIGNATURES["ssaa"]["crender_ssaa_resolve"]
    assert res == C.c_int and len(args) == len(decl.split(",")) == 11
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert declared <= set(re.findall(r" T (crender_\w+)", out))
    # the flag values and the largest factor
    assert (capi.SSAA_U8, capi.SSAA_FLIP) == (1, 2)
    assert re.search(rf"\bCRENDER_SSAA_U8 = {capi.SSAA_U8}u", header)
    assert re.search(rf"\bCRENDER_SSAA_FLIP = {capi.SSAA_FLIP}u", header)
    assert capi.SSAA_MAX == 8 == ssaa_ref.MAX_FACTOR and re.search(rf"\bCRENDER_SSAA_MAX = {capi.SSAA_MAX}\b", header)
    assert capi.ABI_VERSION == 6


def test_ssaa_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit_in_build(_build, "ssaa", ["resolve.hip"], [os.path.join(INCLUDE, "crender_ssaa.h")])
    # the units the other passes pin stay as they were
    assert _build.UNITS["aniso"][0] == ["texaniso.hip"] and _build.UNITS["mip"][0] == ["texmip.hip"]
    # the kernel takes the light's factor from raster_math.h by inclusion
    unit = open(os.path.join(_build.SRC_DIR, "resolve.hip")).read()
    assert "guro_factor(" in unit and "sqrtf" not in unit


def test_ssaa_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    light = (C.c_float * 3)(0, 0, -1)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks first

    def resolve(col=fake, nrm=None, light=None, H=8, W=8, s=2, Y0=0, Y1=4, out=fake, flags=0):
        return L.crender_ssaa_resolve(col, nrm, light, H, W, s, Y0, Y1, out, flags, None)

    def text():
        return L.crender_last_error().decode()

    assert resolve(col=None) == E and "NULL" in text()
    assert resolve(out=None) == E and "NULL" in text()
    for s in (0, -1, 9):
        assert resolve(s=s) == E and "s outside 1 .. 8" in text()
    for kw in (dict(H=0), dict(W=-2), dict(H=9), dict(W=10, s=4, Y1=2), dict(H=7, W=7, s=2)):
        assert resolve(**kw) == E and "multiple of s" in text(), kw
    for kw in (dict(Y0=-1), dict(Y1=5), dict(Y0=2, Y1=2), dict(Y0=3, Y1=1), dict(s=4, Y1=3)):
        assert resolve(**kw) == E and "rows outside the output" in text(), kw
    assert resolve(light=light) == E and "a light without normals" in text()
    assert resolve(nrm=fake) == E and "normals without a light" in text()
    for flags in (4, 8, 0x80000001):
        assert resolve(flags=flags) == E and "unknown flag bits" in text()
    assert text().startswith("crender_ssaa_resolve")


# ---- the model by hand -------------------------------------------------------------------------------------------

def _plane(values, H, W):
    """[H, W, 3] float32 with the given H * W values in every channel, each channel scaled differently."""
    v = np.asarray(values, np.float32).reshape(H, W, 1)
    return np.ascontiguousarray(v * np.float32([1, 2, -1]))


def test_the_order_of_addition_is_row_major_from_the_first_sample():
    d = np.float32
    src = _plane([1e8, 1, -1e8, 1], 2, 2)
    got = ssaa_ref.resolve(src, 2)
    # ((1e8 + 1) + -1e8) + 1: the first 1 is absorbed, the second survives
    assert d(d(d(1e8) + d(1)) + d(-1e8)) + d(1) == d(1.0)
    assert_bit_equal(got, d([[[0.25, 0.5, -0.25]]]), "1e8, 1, -1e8, 1")
    assert_bit_equal(got, ssaa_ref.resolve_by_loops(src, 2), "against the Python loop")
    # any other order gives another value: column-major sums 1e8 + -1e8 first
    assert (d(d(d(1e8) + d(-1e8)) + d(1)) + d(1)) / d(4) == d(0.5)
    rng = np.random.default_rng(3)
    for s, H, W in ((2, 6, 10), (3, 6, 9), (5, 5, 10), (8, 8, 16)):
        src = (rng.uniform(-300, 300, (H, W, 3)) * 10.0 ** rng.integers(-3, 6, (H, W, 3))).astype(np.float32)
        assert_bit_equal(ssaa_ref.resolve(src, s), ssaa_ref.resolve_by_loops(src, s), f"s = {s}")


def test_a_negative_zero_survives_a_factor_of_one():
    src = np.zeros((2, 3, 3), np.float32)
    src[0, 1] = -0.0
    src[1, 2, 0] = -0.0
    got = ssaa_ref.resolve(src, 1)
    assert_bit_equal(got, src, "s = 1 is a bit copy")
    assert np.signbit(got[0, 1]).all() and np.signbit(got).sum() == 4
    assert got is not src and not np.shares_memory(got, src)
    # (a sum that started from +0 would have lost the sign: 0 + -0 = +0)
    assert not np.signbit(np.float32(0.0) + np.float32(-0.0))


def test_a_constant_plane_stays_constant():
    for value in (0.1, 255.0, -37.3, 1e-40):
        for s in (2, 4, 8):
            src = np.full((2 * s, 3 * s, 3), value, np.float32)
            got = ssaa_ref.resolve(src, s)
            assert got.shape == (2, 3, 3)
            assert_bit_equal(got, ssaa_ref.resolve_by_loops(src, s), f"{value} at s = {s}")
            assert (got.view(np.uint32) == got.view(np.uint32)[0, 0]).all()         # every pixel the same bits
    # a value whose multiples up to s * s are exact comes out as itself, through the exact division by s * s
    for s in (2, 4, 8):
        for value in (255.0, -37.0, 0.375):
            src = np.full((s, 2 * s, 3), value, np.float32)
            assert_bit_equal(ssaa_ref.resolve(src, s), np.full((1, 2, 3), value, np.float32), f"{value} at s = {s}")


def test_a_factor_of_three_divides():
    d = np.float32
    # nine samples that sum to 17 exactly: 17 / 9 and 17 * float32(1 / 9) round differently
    assert (d(17) / d(9)).view(np.uint32) == 1072809756 and (d(17) * (d(1) / d(9))).view(np.uint32) == 1072809757
    src = _plane([1, 2, 3, 1, 2, 3, 1, 2, 2], 3, 3)
    got = ssaa_ref.resolve(src, 3)
    assert got[0, 0, 0].view(np.uint32) == 1072809756
    assert_bit_equal(got, (d([17, 34, -17]) / d(9)).reshape(1, 1, 3), "17 / 9")
    # found by search, not by luck: among the integer sums below 200 these differ
    differ = [x for x in range(1, 200) if d(x) / d(9) != d(x) * (d(1) / d(9))]
    assert differ[:5] == [17, 25, 34, 41, 50]


def test_the_uint8_cast_by_hand():
    v = np.float32([-1.5, 255.9, 256.0, 1e10, np.nan, -0.0, 0.99, -255.0, -256.0, 2147483520.0, -2147483648.0,
                    np.inf, -np.inf, 300.7])
    want = np.uint8([255, 255, 0, 0, 0, 0, 0, 1, 0, 128, 0, 0, 0, 44])
    assert np.array_equal(ssaa_ref.present_u8(v), want)
    img = np.arange(24, dtype=np.float32).reshape(4, 2, 3)
    assert np.array_equal(ssaa_ref.present_u8(img, flip_rows=True), img[::-1].astype(np.uint8))
    assert np.array_equal(ssaa_ref.resolve(img, 1, dtype="uint8", flip_rows=True), img[::-1].astype(np.uint8))
    assert np.array_equal(ssaa_ref.resolve(img, 2, dtype="uint8"), ssaa_ref.present_u8(ssaa_ref.resolve(img, 2)))


def test_rows_and_flip_of_the_model():
    rng = np.random.default_rng(5)
    src = rng.uniform(-300, 300, (12, 6, 3)).astype(np.float32)
    full = ssaa_ref.resolve(src, 2)
    part = ssaa_ref.resolve(src, 2, Y0=1, Y1=4)
    assert_bit_equal(part[1:4], full[1:4], "rows inside")
    assert not part[0].any() and not part[4:].any()
    flipped = ssaa_ref.resolve(src, 2, flip_rows=True, Y0=1, Y1=4)
    assert_bit_equal(flipped[2:5], full[1:4][::-1], "row Y lands at Ho - 1 - Y")
    assert not flipped[:2].any() and not flipped[5].any()
    keep = np.full((6, 3, 3), 7.0, np.float32)
    assert ssaa_ref.resolve(src, 2, Y0=2, Y1=3, out=keep) is keep and (keep[:2] == 7).all() and (keep[3:] == 7).all()


def test_the_light_of_the_model_is_the_illumination_then_the_resolve(oracle):
    from cython3dmodelrenderer_amd.illumination import GuroIllumination
    rng = np.random.default_rng(6)
    src = rng.uniform(0, 255, (6, 8, 3)).astype(np.float32)
    nrm = rng.standard_normal((6, 8, 3)).astype(np.float32)
    nrm[2] = 0.0
    light = (0.3, -0.2, 1.0)
    shaded = src.copy()
    GuroIllumination(light).draw_illumination(shaded, nrm)
    assert_bit_equal(ssaa_ref.shade(src, nrm, light), shaded, "the oracle's Guro statements")
    assert_bit_equal(ssaa_ref.resolve(src, 2, normals=nrm, light_direction=light), ssaa_ref.resolve(shaded, 2), "s = 2")
    assert_bit_equal(ssaa_ref.resolve(src, 1, normals=nrm, light_direction=light), shaded, "s = 1 is the pass")


# ---- the protocol on CPU tensors ---------------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._device_planes import DevicePlanes  # noqa: E402

H, W = 8, 12


class FakeFiller(DevicePlanes):
    def __init__(self, row_strip=None):
        super().__init__()
        self.h, self.w = H, W
        self.y0, self.y1 = (0, H) if row_strip is None else row_strip
        self.redo = []             # planes a frame is "rendered again" with, one per _wait_planes call
        self.launches = []         # (factor, light, flags, Y0, Y1) of every _resolve_planes call
        self.readied = self.waits = 0
        self._allocate_planes()

    def _ready_planes(self):
        self.readied += 1

    def _wait_planes(self):
        self.waits += 1
        if not self.redo:
            return False
        self.color_buffer.copy_(self.redo.pop(0))
        return True

    def _allocate_planes(self, track_winner=False):
        self.z_buffer = torch.full((H, W), 1e6, dtype=torch.float32)
        self.color_buffer = torch.zeros((H, W, 3), dtype=torch.float32)
        self.normals_buffer = torch.zeros((H, W, 3), dtype=torch.float32)

    def _pinned_like(self, buf):
        return torch.full(tuple(buf.shape), -1.0, dtype=buf.dtype)

    def _resolve_planes(self, out, factor, light, flags, Y0, Y1):
        self.launches.append((factor, light, flags, Y0, Y1))
        ssaa_ref.resolve(self.color_buffer.numpy(), factor, dtype="uint8" if flags & 1 else "float32",
                         flip_rows=bool(flags & 2), Y0=Y0, Y1=Y1, out=out.numpy())


def _random_plane(seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-300, 300, (H, W, 3)).astype(np.float32))


def test_an_edit_made_in_a_view_is_resolved():
    f = FakeFiller()
    f.color_buffer.copy_(_random_plane(1))
    view = f.get_color_buffer()
    fresh, exposed = f._host_fresh, f._host_exposed
    assert fresh and exposed
    view[0:2, 0:2] = 1000.0
    f.waits = 0
    out = f.resolve(2)
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (4, 6, 3)
    assert (out[0, 0] == 1000.0).all()
    assert (f.color_buffer[0:2, 0:2] == 1000.0).all()          # carried up first
    assert_bit_equal(out.numpy(), ssaa_ref.resolve(view, 2), "the edited view, resolved")
    assert f.launches == [(2, None, 0, 0, 4)] and f.waits == 1
    # the planes are only read: the views are as fresh as they were, and the edit is not pushed twice
    assert f._host_fresh is fresh and not f._host_exposed
    assert f.get_color_buffer() is view and (view[0, 0] == 1000.0).all()
    # a new tensor per call, the arguments handed through
    again = f.resolve(4, light_direction=np.float32([0, 0, -1]), dtype="uint8", flip_rows=True)
    assert again is not out and again.dtype == torch.uint8 and tuple(again.shape) == (2, 3, 3)
    assert f.launches[1] == (4, [0.0, 0.0, -1.0], 3, 0, 2)
    assert np.array_equal(again.numpy(), ssaa_ref.resolve(view, 4, dtype="uint8", flip_rows=True))


def test_a_frame_rendered_again_is_resolved_again_into_the_same_tensor():
    f = FakeFiller()
    f.color_buffer.copy_(_random_plane(2))
    second = _random_plane(3)
    f.redo = [second.clone()]
    out = f.resolve(2)
    assert len(f.launches) == 2 and f.waits == 2 and not f.redo
    assert_bit_equal(out.numpy(), ssaa_ref.resolve(second.numpy(), 2), "the frame that stays")
    f.launches.clear()
    f.waits = 0
    f.resolve(1)
    assert len(f.launches) == 1 and f.waits == 1


def test_a_row_strip_resolves_its_rows_and_leaves_zeros():
    f = FakeFiller(row_strip=(2, 6))
    f.color_buffer.copy_(_random_plane(4))
    out = f.resolve(2)
    assert f.launches == [(2, None, 0, 1, 3)]
    want = ssaa_ref.resolve(f.color_buffer.numpy(), 2)
    assert_bit_equal(out.numpy()[1:3], want[1:3], "the strip's rows")
    assert not out[0].any() and not out[3].any()
    with pytest.raises(ValueError, match="row strip"):
        f.resolve(4)                     # 8 x 12 divides, rows 2 .. 6 do not
    assert len(f.launches) == 1


def test_bad_arguments_name_their_cause():
    f = FakeFiller()
    for bad in (0, 9, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="factor must be an int from 1 to 8"):
            f.resolve(bad)
    for s in (3, 5, 7, 8):               # 8 x 12 is a multiple of 1, 2, 4 in both directions
        with pytest.raises(ValueError, match=f"not a multiple of factor={s}"):
            f.resolve(s)
    for bad in ("float16", "u8", None, np.uint8):
        with pytest.raises(ValueError, match="dtype must be 'float32' or 'uint8'"):
            f.resolve(2, dtype=bad)
    assert f.launches == [] and f.waits == 0
    sig = inspect.signature(DevicePlanes.resolve)
    assert list(sig.parameters)[1:] == ["factor", "light_direction", "dtype", "flip_rows"]
    assert [p.default for p in sig.parameters.values()][2:] == [None, "float32", False]


def test_both_gpu_fillers_and_the_renderer_carry_it():
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller
    from cython3dmodelrenderer_amd.pixel_buffer_filler.edge_only import EdgeOnlyPixelBufferFiller
    from cython3dmodelrenderer_amd.renderer import Renderer
    assert AdvancedPixelBufferFiller.resolve is DevicePlanes.resolve is EdgeOnlyPixelBufferFiller.resolve
    sig = inspect.signature(Renderer.__init__)
    assert list(sig.parameters)[-1] == "supersample" and sig.parameters["supersample"].default is None
    with pytest.raises(ValueError, match="supersample"):
        Renderer(types.SimpleNamespace(), None, supersample=2)        # a filler without planes on the device
    assert Renderer(types.SimpleNamespace(), None).supersample is None
