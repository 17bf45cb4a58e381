"""Bloom and tone mapping without a GPU: the header against the binding and the library, the unit's place in the build
tables, the entry point's argument checks, the host model the GPU tests compare with (tests/bloom_ref.py) pinned by
identities, against its own float64 evaluation and on the pinned scenes; ``DevicePlanes.bloom``'s protocol on CPU tensors,
``Renderer(bloom=...)`` through recording fillers, and ``bloom.gaussian``."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bloom_ref
from pass_scenes import Frame, capi, recording_filler, soups_fixture, trex_fixture  # noqa: F401 (fixtures)
from ssaa_ref import present_u8
from util import assert_bit_equal, other_symbols, own_unit_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "crender_bloom"
_vp, _i32, _f = C.c_void_p, C.c_int, C.c_float
BLOOM_ARGTYPES = [_vp, _f, C.POINTER(C.c_float), _i32, _f, _f, _f, _f, _vp, _vp, _i32, _i32, _i32, _i32, C.c_uint, _vp]
INF, NAN = float("inf"), float("nan")


# ---- the host side of the ABI ----------------------------------------------------------------------------------

def test_bloom_symbol_is_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "crender_bloom.h")).read()
    declared = set(re.findall(r"CRENDER_API[^;(]*?\b(crender_\w+)\s*\(", header))
    assert declared == set(capi.UNIT_SIGNATURES["bloom"]) == {ENTRY}
    assert not declared & other_symbols(capi, "bloom")
    res, args = capi.UNIT_SIGNATURES["bloom"][ENTRY]
    assert res == C.c_int and args == BLOOM_ARGTYPES == getattr(capi.load(), ENTRY).argtypes
    decl = re.search(r"CRENDER_API int " + ENTRY + r"\((.*?)\);", header, re.S).group(1)
    params = [" ".join(a.split()) for a in decl.split(",")]
    assert params == ["const float *d_src", "float threshold", "const float *weights", "int radius", "float intensity",
                      "float exposure", "float inv_white2", "float clamp", "float *d_scratch", "void *d_out", "int H", "int W",
                      "int y0", "int y1", "unsigned flags", "void *stream"]
    assert len(params) == len(args) == 16
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.lib_path()], text=True)
    assert ENTRY in set(re.findall(r" T (crender_\w+)", out))
    top = int(re.search(r"#define CRENDER_BLOOM_MAX_RADIUS (\d+)", header).group(1))
    assert top == capi.BLOOM_MAX_RADIUS == bloom_ref.MAX_RADIUS == 32
    flags = {n: int(v) for n, v in re.findall(r"#define CRENDER_BLOOM_(U8|FLIP|REINHARD|GAMMA2) (\d+)u", header)}
    assert flags == dict(U8=capi.BLOOM_U8, FLIP=capi.BLOOM_FLIP, REINHARD=capi.BLOOM_REINHARD, GAMMA2=capi.BLOOM_GAMMA2) \
        == dict(U8=1, FLIP=2, REINHARD=4, GAMMA2=8)
    # three planes of the largest staged tile stay below the 64 KB that need no launch attribute
    assert 3 * 32 * (32 + 64) * 4 == 36864 and 36864 + 4 * 4 < 65536
    assert capi.ABI_VERSION == 6 and capi.load().crender_abi_version() == 6
    assert np.float32(1.0 / 255.0).view(np.uint32) == 0x3B808081 and "0x3B808081" in header


def test_bloom_sources_are_built_and_stay_out_of_the_profile_fingerprint():
    from cython3dmodelrenderer_amd import _build
    unit = new = own_unit_source(_build, "bloom", "bloom.hip", "crender_bloom.h")
    head = "// ---- bloom (crender_bloom) ----"
    assert unit.count(head) == 1
    assert unit.index(head) < unit.index("void k_bloom_rows") < unit.index("void k_bloom_finish") \
        < unit.index("int crender_bloom(")
    # a unit of its own: its namespace and its entry point, the passes' frame from the shared header as it is
    assert new.count("namespace {") == 1 and new.count('extern "C" {') == 1
    for name in ("tile_lane(", "tile_origin(", "tile_grid(", "frame_checks(", "rows_check(", "arg_error(", "wave_any("):
        assert name in new and not re.search(r"CR_DEV[^\n]*\b" + re.escape(name), unit), name
    assert "CR_DEV" not in new and "asm" not in new
    code = "\n".join(line.split("//")[0] for line in new.splitlines())
    for banned in ("expf", "powf", "logf", "exp2f", "log2f"):
        assert banned not in code, banned
    # one staging barrier and one at the end of a tile, in each kernel; no tap divides or takes a root
    rows = new[new.index("void k_bloom_rows"):new.index("// crender_present_u8's cast")]
    finish = new[new.index("void k_bloom_finish"):new.index("}  // namespace")]
    for body in (rows, finish):
        assert "extern __shared__" in body and body.count("__syncthreads()") == 2 and "bloom_walk(" in body
    walk = code[code.index("void bloom_walk"):code.index("void k_bloom_rows")]
    assert "/" not in walk and "sqrtf" not in walk
    assert finish.count("template <bool U8>") == 0 and new.count("template <bool U8>") == 1       # one instance per store
    assert new.index("frame_checks(E") < new.index("rows_check(E") < new.index("is NULL") < new.index("radius is not") \
        < new.index("a weight is not finite") < new.index("threshold is") < new.index("intensity is not") \
        < new.index("exposure is not") < new.index("inv_white2 is") < new.index("clamp is NaN") < new.index("unknown flag bits") \
        < new.index("hipLaunchKernelGGL")


def test_bloom_argument_errors_without_a_gpu(capi):
    L = capi.load()
    E = capi.EINVAL
    fake, other, third = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)     # never dereferenced
    good = (C.c_float * 33)(*([0.25] * 33))

    def run(src=fake, threshold=255.0, w=good, R=8, intensity=1.0, exposure=1.0, iw2=0.0, clamp=INF, scratch=other, out=third,
            H=8, W=8, y0=0, y1=8, flags=0):
        return L.crender_bloom(src, threshold, w, R, intensity, exposure, iw2, clamp, scratch, out, H, W, y0, y1, flags, None)

    def text():
        return L.crender_last_error().decode()

    for kw in (dict(H=0), dict(W=-2), dict(H=-2 ** 31)):
        assert run(**kw) == E and "H or W is below 1" in text(), kw
    for kw in (dict(y0=-1), dict(y1=9), dict(y0=3, y1=3), dict(y0=5, y1=2)):
        assert run(**kw) == E and "rows outside the frame" in text(), kw
    for kw in (dict(src=None), dict(w=None), dict(scratch=None), dict(out=None)):
        assert run(**kw) == E and "d_src, weights, d_scratch or d_out is NULL" in text(), kw
    for bad in (0, -1, 33, 2 ** 31 - 1, -2 ** 31):
        assert run(R=bad) == E and "radius is not 1 .. 32" in text(), bad
    for at in (0, 3, 8):
        for bad in (NAN, INF, -INF):
            w = (C.c_float * 33)(*([0.25] * 33))
            w[at] = bad
            assert run(w=w) == E and "a weight is not finite" in text(), (at, bad)
    w = (C.c_float * 33)(*([0.25] * 33))
    w[9] = NAN                                  # beyond radius: not looked at
    assert run(w=w, threshold=-1.0) == E and "threshold is" in text()
    for bad in (-1e-9, -INF, NAN):
        assert run(threshold=bad) == E and "threshold is negative or NaN" in text(), bad
    for bad in (-1e-9, NAN, INF, -INF):
        assert run(intensity=bad) == E and "intensity is not finite and 0 or above" in text(), bad
        assert run(exposure=bad) == E and "exposure is not finite and 0 or above" in text(), bad
    for bad in (-1e-9, -INF, NAN):
        assert run(iw2=bad) == E and "inv_white2 is negative or NaN" in text(), bad
    assert run(clamp=NAN) == E and "clamp is NaN" in text()
    for flags in (16, 32, 0x80000000, 0xFFFFFFF0):
        assert run(flags=flags) == E and "unknown flag bits" in text(), flags
    for kw in (dict(out=fake), dict(out=other), dict(scratch=fake)):
        assert run(**kw) == E and "are not three planes" in text(), kw
    assert text().startswith("crender_bloom: ")
    # the order
    bad = dict(H=0, y0=9, src=None, R=0, w=w, threshold=-1.0, intensity=-1.0, exposure=-1.0, iw2=-1.0, clamp=NAN, flags=16,
               out=fake)
    w[0] = NAN
    for drop, word in (("H", "H or W is below 1"), ("y0", "rows outside"), ("src", "is NULL"), ("R", "radius is not"),
                       ("w", "a weight is not finite"), ("threshold", "threshold is"), ("intensity", "intensity is not"),
                       ("exposure", "exposure is not"), ("iw2", "inv_white2 is"), ("clamp", "clamp is NaN"),
                       ("flags", "unknown flag bits"), ("out", "are not three planes")):
        assert run(**bad) == E and word in text(), drop
        del bad[drop]
    # what is allowed: a threshold and a clamp of +inf, a clamp of -inf, an infinite inv_white2, zero weights.  Such a call
    # goes on to its launch; it is made here only where no device could run it, and ends in the runtime's refusal.
    if not torch.cuda.is_available():
        zero = (C.c_float * 2)(0.0, -0.0)
        assert run(threshold=INF, clamp=-INF, iw2=INF, w=zero, R=1, intensity=0.0, exposure=0.0, flags=15) in (capi.OK, capi.EHIP)


# ---- identities of the model -----------------------------------------------------------------------------------

def _odd_image(seed=5, H=37, W=45, top=400.0):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, top, (H, W, 3)).astype(np.float32)
    img[3, 4] = np.float32([-0.0, np.nan, 17.0])
    img[5, 6].view(np.uint32)[:] = [0x7FC00123, 0xFFC00001, 0x80000000]      # NaN payloads and a -0
    img[7, 8] = np.float32([-3.0, -np.inf, -0.0])
    return img


def test_intensity_zero_and_a_high_threshold_copy():
    img = _odd_image()
    for R in (1, 8, 32):
        c = {}
        assert_bit_equal(bloom_ref.bloom(img, threshold=100.0, radius=R, intensity=0.0, counts=c), img, f"intensity 0, radius {R}")
        assert c["bright"] > 1000
        c = {}
        assert_bit_equal(bloom_ref.bloom(img, threshold=400.0, radius=R, counts=c), img, f"a threshold above every pixel, radius {R}")
        assert c == dict(bright=0, copied=37 * 45, glow=0)
    assert_bit_equal(bloom_ref.bloom(img, threshold=INF), img, "a threshold of +inf")
    # a clamp of +inf and None are the same; a NaN passes the clamp
    assert_bit_equal(bloom_ref.bloom(img, threshold=400.0, clamp=INF), img, "clamp +inf")
    cut = bloom_ref.bloom(img, threshold=400.0, clamp=200.0)
    assert np.nanmax(cut) == 200 and np.isnan(cut[3, 4, 1]) and cut[5, 6].view(np.uint32)[1] == 0xFFC00001


def test_a_single_bright_pixel_gives_the_outer_product_of_the_weights():
    for R, w in ((1, np.float32([0.5, 0.25])), (8, bloom_ref.gaussian(8)), (32, bloom_ref.gaussian(32)),
                 (3, np.float32([0.5, -0.125, 0.0, 2.0]))):
        H = W = 2 * R + 9
        img = np.zeros((H, W, 3), np.float32)
        cy, cx = R + 3, R + 5
        img[cy, cx] = np.float32([300.0, 150.0, 75.0])
        c, hb = {}, np.full_like(img, np.nan)
        out = bloom_ref.bloom(img, threshold=255.0, weights=w, intensity=0.5, counts=c, scratch=hb)
        k = np.float32(300.0) - np.float32(255.0)
        q = k / np.float32(300.0)
        bright = img[cy, cx] * q
        assert bright[0] == np.float32(300.0) * q and abs(float(bright[0]) - 45.0) < 1e-4        # m q = k up to rounding
        full = np.concatenate([w[:0:-1], w])                                      # w[|d|], d = -R .. R
        # one product per direction: 0 + w b is w b exactly, and so is the sum of one non-zero term
        want_hb = np.zeros_like(img)
        want_hb[cy, cx - R:cx + R + 1] = full[:, None] * bright[None, :]
        assert_bit_equal(hb, want_hb, f"hb, radius {R}")
        glow = np.zeros_like(img)
        glow[cy - R:cy + R + 1, cx - R:cx + R + 1] = full[:, None, None] * want_hb[cy, cx - R:cx + R + 1][None]
        want = np.where(glow != 0, img + np.float32(0.5) * glow, img)
        assert_bit_equal(out, want, f"the outer product, radius {R}")
        nonzero = int(((full[:, None] * full[None, :]) != 0).sum())
        assert c == dict(bright=1, copied=H * W - nonzero, glow=nonzero)
        if R == 3:
            assert nonzero == 25                                                  # the zero weight's row and column are copied


def test_the_glow_sums_to_the_bright_values_for_normalised_weights():
    rng = np.random.default_rng(11)
    img = np.zeros((120, 130, 3), np.float32)
    img[40:80, 40:90] = rng.uniform(0.0, 600.0, (40, 50, 3)).astype(np.float32)       # out of the edges' reach at radius 32
    for R in (1, 8, 32):
        out = bloom_ref.bloom(img, threshold=255.0, radius=R)
        bright = bloom_ref.bright_pass(img, 255.0)[0]
        total, glow = bright.astype(np.float64).sum((0, 1)), (out.astype(np.float64) - img).sum((0, 1))
        # the weights sum to 1 within 2 R + 1 roundings of 2^-25; every pixel's two sums and the composite round as well
        assert np.all(total > 1e5) and np.all(np.abs(glow - total) <= total * 4e-5), (R, total, glow)
        w = bloom_ref.gaussian(R).astype(np.float64)
        assert abs(w[0] + 2 * w[1:].sum() - 1) <= (2 * R + 1) * 2.0 ** -25


def test_tone_mapping_identities():
    img = _odd_image(top=2000.0)
    # Reinhard with white = inf stays below 255, whatever comes in; without it 2000 stays 2000
    plain = bloom_ref.bloom(img, threshold=INF, tonemap="reinhard")
    assert np.nanmax(plain) < 255 and np.nanmax(plain) > 200 and np.nanmax(bloom_ref.bloom(img, threshold=INF)) > 1990
    assert plain[7, 8, 0] == 0 and plain[7, 8, 1] == 0 and np.signbit(plain[7, 8, 2]) == np.signbit(np.float32(0.0))
    assert bloom_ref.tone(np.float32([np.nan]), tonemap="reinhard")[0] == 0      # a > 0 fails: rule 5 gives 0
    # a white point maps itself to 255 (up to rounding) and what lies above it above 255, which the clamp cuts
    white = bloom_ref.tone(np.float32([1000.0, 2000.0]), tonemap="reinhard", white=1000.0 / 255.0)
    assert abs(float(white[0]) - 255.0) < 1e-3 and white[1] > 255
    assert bloom_ref.tone(np.float32([2000.0]), tonemap="reinhard", white=1000.0 / 255.0, clamp=255.0)[0] == 255
    assert bloom_ref.inv_white2(INF) == 0 and bloom_ref.inv_white2(2.0) == np.float32(0.25)
    # gamma 2 of the squared image returns it (values a of multiples of 1/255 in 0 .. 1: v = 255 a^2)
    a = (np.arange(256, dtype=np.float32) / np.float32(255.0))
    sq = np.tile(((a * a) * np.float32(255.0))[:, None, None], (1, 2, 3))
    back = bloom_ref.bloom(sq, threshold=INF, gamma=2)
    assert np.abs(back - np.tile((a * np.float32(255.0))[:, None, None], (1, 2, 3))).max() <= 255 * 3 * 2.0 ** -24
    assert back[0, 0, 0] == 0 and back[255, 0, 0] == 255
    # an exposure other than 1 alone runs the stage; 1 does not (negative values and -0 survive)
    assert_bit_equal(bloom_ref.bloom(img, threshold=INF, exposure=1.0), img, "exposure 1")
    half = bloom_ref.bloom(img, threshold=INF, exposure=0.5)
    assert half[7, 8, 0] == 0 and abs(float(half[10, 10, 0]) - 0.5 * float(img[10, 10, 0])) < 1e-3
    # uint8 is numpy's cast of the float result, clamped at 255 unless told otherwise; flipped rows are the rows flipped
    img = _odd_image(top=330.0)
    for kw in (dict(), dict(tonemap="reinhard", gamma=2), dict(clamp=300.0)):
        f32 = bloom_ref.bloom(img, threshold=250.0, radius=4, **dict(dict(clamp=255.0), **kw))
        u8 = bloom_ref.bloom(img, threshold=250.0, radius=4, dtype="uint8", **kw)
        assert u8.dtype == np.uint8 and np.array_equal(u8, present_u8(f32))
        ok = ~np.isnan(f32) & (f32 >= 0) & (f32 < 256)
        assert np.array_equal(u8[ok], f32[ok].astype(np.uint8)) and ok.sum() > 3000
        assert np.array_equal(bloom_ref.bloom(img, threshold=250.0, radius=4, dtype="uint8", flip_rows=True, **kw), u8[::-1])
    f32 = bloom_ref.bloom(img, threshold=250.0, radius=4, clamp=300.0)
    u8 = bloom_ref.bloom(img, threshold=250.0, radius=4, dtype="uint8", clamp=300.0)
    assert (f32 == 300).sum() > 100 and (u8[f32 == 300] == 44).all()              # 300 -> 44: the low byte


def test_a_strip_does_not_see_across_its_edge():
    img = _odd_image(seed=9, H=60, W=41)
    sentinel = np.full_like(img, -7.0)
    hb = np.full_like(img, -9.0)
    strip = bloom_ref.bloom(img, threshold=200.0, radius=8, y0=20, y1=50, out=sentinel.copy(), scratch=hb)
    assert (strip[:20] == -7).all() and (strip[50:] == -7).all() and (hb[:20] == -9).all() and (hb[50:] == -9).all()
    poisoned = img.copy()
    poisoned[:20], poisoned[50:] = 1e9, np.nan
    assert_bit_equal(bloom_ref.bloom(poisoned, threshold=200.0, radius=8, y0=20, y1=50, out=sentinel.copy()), strip,
                     "rows outside the strip are not read")
    whole = bloom_ref.bloom(img, threshold=200.0, radius=8)
    assert_bit_equal(whole[28:42], strip[28:42], "rows out of the edge's reach")
    assert (whole[20] != strip[20]).any()
    zeros = bloom_ref.bloom(img, threshold=200.0, radius=8, y0=20, y1=50)
    assert not zeros[:20].any() and not zeros[50:].any()
    flipped = bloom_ref.bloom(img, threshold=200.0, radius=8, y0=20, y1=50, flip_rows=True)
    assert_bit_equal(flipped, zeros[::-1], "a flipped strip")


def test_gaussian_is_the_models_table():
    from cython3dmodelrenderer_amd import bloom
    for R, sigma in ((1, None), (8, None), (32, None), (8, 1.0), (32, 100.0)):
        w = bloom.gaussian(R, sigma)
        assert w.dtype == np.float32 and w.shape == (R + 1,) and np.isfinite(w).all() and (np.diff(w) <= 0).all()
        assert_bit_equal(w, bloom_ref.gaussian(R, sigma), f"gaussian({R}, {sigma})")
        s = R / 3.0 if sigma is None else sigma
        k = np.arange(R + 1, dtype=np.float64)
        e = np.exp(-k * k / (2 * s * s))
        assert np.allclose(w, e / (e[0] + 2 * e[1:].sum()), rtol=1e-6, atol=1e-45)
    for bad in (0, 33, -1, 8.0, True, None):
        with pytest.raises(ValueError, match="radius must be an int from 1 to 32, got " + re.escape(repr(bad))):
            bloom.gaussian(bad)
    for bad in (0, -1.0, NAN, INF, "2", True):
        with pytest.raises(ValueError, match="sigma must be a finite number above 0, got " + re.escape(repr(bad))):
            bloom.gaussian(8, bad)
    assert bloom.MAX_RADIUS == 32 and bloom.KEYS[0] == "threshold" and "source" not in bloom.KEYS


# ---- the oracle's frames: the pinned scenes and float64 ---------------------------------------------------------

class _Frame(Frame):
    def run(self, **kw):
        return bloom_ref.bloom(self.cam.color_buffer, **kw)


SOUPS = {51: (4000, 200, 173, (1.0, 40.0)), 71: (3000, 256, 256, (3.0, 50.0))}       # test_wire_pass_cpu.py's scenes

soups = soups_fixture(_Frame, SOUPS)
trex = trex_fixture(_Frame)


def test_the_pinned_scenes(trex, soups):
    """T-Rex and the soup of seed 71 (pass_scenes.Soup's arrays, the GPU tests' soup) at 256^2: the threshold is the 0.9
    quantile of the largest channel over the frame, so a tenth of the pixels is bright.  On T-Rex more than a twentieth
    is copied and more than a twentieth glows at every radius.  The soup covers its whole frame: at radius 1 and 8 the
    three shares hold; at radius 32 a tenth of the pixels, spread over the frame, reaches every pixel, and no threshold
    leaves a twentieth bright AND a twentieth copied: copied is pinned at 0 there."""
    for name, f in (("trex", trex), ("soup", soups[71])):
        largest = f.cam.color_buffer.max(2)
        thr = float(np.float32(np.quantile(largest, 0.9)))
        print(f"{name}: the 0.9 quantile of the largest channel is {thr!r}")
        assert thr == bloom_ref.PINNED_THRESHOLD[name]
        for R in (1, 8, 32):
            c = {}
            out = f.run(threshold=thr, radius=R, counts=c)
            print(f"{name}, radius {R}: {c}")
            assert (c["bright"], c["copied"], c["glow"]) == bloom_ref.PINNED_COUNTS[name, R]
            n = 256 * 256
            assert c["copied"] + c["glow"] == n and c["bright"] >= 0.05 * n and c["glow"] >= 0.05 * n
            if (name, R) == ("soup", 32):
                assert c["copied"] == 0
            else:
                assert c["copied"] >= 0.05 * n
            changed = (out.view(np.uint32) != f.cam.color_buffer.view(np.uint32)).any(2)
            # (a glow below half an ulp of its pixel leaves the bits: a few pixels at the rim)
            assert 0.99 * c["glow"] <= changed.sum() <= c["glow"] and not np.isnan(out).any()
            assert (out >= f.cam.color_buffer).all()                              # a glow only adds
    # the soup at radius 32 with as few bright pixels as the twentieth allows: still nothing is copied
    c = {}
    soups[71].run(threshold=float(np.float32(np.quantile(soups[71].cam.color_buffer.max(2), 0.95))), radius=32, counts=c)
    assert c["bright"] == 3277 >= 0.05 * 256 * 256 and c["copied"] == 0


def test_float32_against_float64(trex, soups):
    """The same statements in float64 from the same float32 inputs (the image, the weights, the threshold), every pixel of
    the three frames, radius 8 and 32 at the 0.9 quantile, plain and through Reinhard and gamma 2; colours are 0 .. 255.
    A pixel is its source plus two nested sums of up to 65 products of values up to 255 with weights that sum to 1: each
    sum's roundings are 2^-24 of a partial sum below 255, up to 2 * 65 of them, but they do not align.  The bound is ten
    times the largest measured difference: the margin is for frames not measured.  A check of the model's statements,
    not a bound on the kernel, which is held to bit equality with the float32 model."""
    worst = 0.0
    for name, f in (("trex", trex), ("soup51", soups[51]), ("soup71", soups[71])):
        thr = float(np.float32(np.quantile(f.cam.color_buffer.max(2), 0.9)))
        for kw in (dict(radius=8), dict(radius=32), dict(radius=8, tonemap="reinhard", gamma=2, exposure=1.5)):
            o32 = f.run(threshold=thr, **kw)
            o64 = f.run(threshold=thr, compute=np.float64, **kw)
            assert o32.dtype == np.float32 and o64.dtype == np.float64 and not np.isnan(o64).any()
            diff = float(np.abs(o32.astype(np.float64) - o64).max())
            print(f"{name}, {kw}: largest |out - out64| = {diff:.3e}")
            worst = max(worst, diff)
    print(f"largest |out - out64| over the frames = {worst:.3e} (bound {10 * bloom_ref.F64_MEASURED:.3e})")
    assert 0 < worst <= 10 * bloom_ref.F64_MEASURED


# ---- the Python layer, on CPU tensors --------------------------------------------------------------------------

from cython3dmodelrenderer_amd.pixel_buffer_filler._device_planes import DevicePlanes  # noqa: E402


def _model_of(call, src, y0, y1, **kw):
    """The model's result of a recorded ``bloom.Call``."""
    from cython3dmodelrenderer_amd import _capi
    return bloom_ref.bloom(src, threshold=call.threshold, weights=call.weights, intensity=call.intensity, exposure=call.exposure,
                           tonemap="reinhard" if call.flags & _capi.BLOOM_REINHARD else None, inv_w2=call.inv_white2,
                           gamma=2 if call.flags & _capi.BLOOM_GAMMA2 else 1, clamp=call.clamp,
                           dtype="uint8" if call.flags & _capi.BLOOM_U8 else "float32",
                           flip_rows=bool(call.flags & _capi.BLOOM_FLIP), y0=y0, y1=y1, **kw)


class FakeFiller(DevicePlanes):
    """``DevicePlanes``' protocol on CPU tensors; the launch is recorded and answered by the host model."""
    device = "cpu"

    def __init__(self, color, row_strip=None):
        super().__init__()
        self.h, self.w = color.shape[:2]
        self.y0, self.y1 = (0, self.h) if row_strip is None else row_strip
        self.color_buffer = torch.from_numpy(color.copy())
        self.z_buffer = torch.zeros((self.h, self.w))
        self.normals_buffer = torch.zeros((self.h, self.w, 3))
        self.events = []
        self.redo = 0

    def _ready_planes(self):
        self.events.append("ready")

    def _wait_planes(self):
        self.events.append("wait")
        if self.redo:
            self.redo -= 1
            return True
        return False

    def _push_host_edits(self):
        self.events.append("push")
        super()._push_host_edits()

    def _pinned_like(self, buf):
        return torch.empty(tuple(buf.shape), dtype=buf.dtype)

    def _bloom_planes(self, src, scratch, out, call, y0, y1):
        self.events.append(("crender_bloom", call, y0, y1))
        assert out is not src and scratch is not src and scratch is not out and scratch.shape == src.shape
        assert scratch.dtype == torch.float32 and out.shape == src.shape
        assert all(type(v) is float for v in (call.threshold, call.intensity, call.exposure, call.inv_white2, call.clamp))
        assert type(call.radius) is int and call.weights.dtype == np.float32 and len(call.weights) == call.radius + 1
        out.copy_(torch.from_numpy(_model_of(call, src.numpy(), y0, y1, out=out.numpy().copy(), scratch=scratch.numpy())))

    def launches(self):
        return [e for e in self.events if isinstance(e, tuple)]


@pytest.fixture(scope="module")
def hot():
    """A frame with highlights above 255, a -0 and NaNs."""
    return _odd_image(seed=21, H=70, W=50, top=330.0)


def test_bloom_returns_a_new_tensor_and_leaves_the_views_as_they_were(hot):
    f = FakeFiller(hot)
    out = f.bloom()
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (70, 50, 3)
    assert out.data_ptr() != f.color_buffer.data_ptr()
    # the plane completed (the getter), the edits carried up, the launch, the settle
    assert [e if isinstance(e, str) else e[0] for e in f.events] == ["ready", "push", "ready", "crender_bloom", "wait"]
    call, y0, y1 = f.launches()[0][1:]
    assert (y0, y1) == (0, 70) and call.threshold == 255.0 and call.radius == 8 and call.intensity == 1.0 and call.exposure == 1.0
    assert call.inv_white2 == 0.0 and call.clamp == INF and call.flags == 0 and call.dtype == "float32"
    assert_bit_equal(call.weights, bloom_ref.gaussian(8), "the default table")
    c = {}
    want = bloom_ref.bloom(hot, counts=c)
    assert c["bright"] > 100 and c["glow"] > c["bright"]
    assert_bit_equal(out.numpy(), want, "the model's image")
    assert not f._host_fresh and not f._host_exposed                     # nobody asked for a view: as stale as before
    assert_bit_equal(f.color_buffer.numpy(), hot, "the colour plane is only read")
    sig = inspect.signature(DevicePlanes.bloom)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == \
        [("threshold", 255.0), ("radius", 8), ("weights", None), ("intensity", 1.0), ("exposure", 1.0), ("tonemap", None),
         ("white", INF), ("gamma", 1), ("clamp", None), ("dtype", "float32"), ("flip_rows", False), ("source", None)]
    # the scratch plane is kept per shape
    kept = f._bloom_scratch[(70, 50)]
    again = f.bloom(threshold=300.0, radius=2)
    assert again is not out and f._bloom_scratch[(70, 50)] is kept and list(f._bloom_scratch) == [(70, 50)]
    hb = np.zeros_like(hot)
    bloom_ref.bloom(hot, threshold=300.0, radius=2, scratch=hb)
    assert_bit_equal(kept.numpy(), hb, "the scratch plane holds hb")
    # an edit made in a view is carried up first and glows; the views stay fresh
    view = f.get_color_buffer()
    assert f._host_fresh and f._host_exposed
    view[30:34, 20:24] = np.float32([1000.0, 10.0, 500.0])
    f.events.clear()
    lit = f.bloom()
    assert f._host_fresh and not f._host_exposed and f.events[:2] == ["ready", "push"]
    edited = hot.copy()
    edited[30:34, 20:24] = np.float32([1000.0, 10.0, 500.0])
    assert_bit_equal(lit.numpy(), bloom_ref.bloom(edited), "over the edited colours")
    assert f.get_color_buffer() is view
    # a frame rendered again meanwhile is bloomed again, into the same tensor
    f.events.clear()
    f.redo = 1
    f.bloom()
    assert [e if isinstance(e, str) else e[0] for e in f.events] == ["ready", "push", "ready", "crender_bloom", "wait", "ready",
                                                                     "crender_bloom", "wait"]


def test_bloom_options_reach_the_entry(hot):
    from cython3dmodelrenderer_amd import _capi
    f = FakeFiller(hot)
    out = f.bloom(threshold=200, radius=3, intensity=2, exposure=1.5, tonemap="reinhard", white=4.0, gamma=2, dtype="uint8",
                  flip_rows=True)
    call = f.launches()[-1][1]
    assert call.flags == _capi.BLOOM_U8 | _capi.BLOOM_FLIP | _capi.BLOOM_REINHARD | _capi.BLOOM_GAMMA2 == 15
    assert call.clamp == 255.0 and call.inv_white2 == 0.0625 and call.radius == 3 and call.threshold == 200.0
    assert out.dtype == torch.uint8
    want = bloom_ref.bloom(hot, threshold=200.0, radius=3, intensity=2.0, exposure=1.5, tonemap="reinhard", white=4.0, gamma=2,
                           dtype="uint8", flip_rows=True)
    assert np.array_equal(out.numpy(), want) and want.max() > 200 and len(np.unique(want)) > 100
    # uint8 with a clamp of its own keeps it; float32 without one has none; "none" is no operator
    f.bloom(dtype="uint8", clamp=300.0)
    assert f.launches()[-1][1].clamp == 300.0
    f.bloom(clamp=-INF, tonemap="none")
    assert f.launches()[-1][1].clamp == -INF and f.launches()[-1][1].flags == 0
    assert f.bloom(white=1e-30).dtype == torch.float32 and f.launches()[-1][1].inv_white2 == INF
    # an explicit table fixes the radius, whatever `radius` says
    table = [0.5, 0.2, 0.05]
    f.bloom(weights=table, radius=20)
    call = f.launches()[-1][1]
    assert call.radius == 2
    assert_bit_equal(call.weights, np.float32(table), "the table")
    f.bloom(weights=np.float64([1.0] + [0.0] * 32))
    assert f.launches()[-1][1].radius == 32
    f.bloom(weights=torch.tensor([0.25, 0.25]))
    assert f.launches()[-1][1].radius == 1


def test_bloom_on_a_row_strip_and_on_a_source(hot):
    g = FakeFiller(hot, row_strip=(17, 55))
    strip = g.bloom(radius=4).numpy()
    assert g.launches()[-1][2:] == (17, 55)
    assert not strip[:17].any() and not strip[55:].any()
    assert_bit_equal(strip[17:55], bloom_ref.bloom(hot, radius=4, y0=17, y1=55)[17:55], "the strip's rows")
    flipped = g.bloom(radius=4, flip_rows=True).numpy()
    assert_bit_equal(flipped, strip[::-1], "the strip, flipped")
    # a source of another size: all of its rows, the filler's planes and strip not looked at
    other = torch.from_numpy(_odd_image(seed=22, H=33, W=91, top=300.0))
    g.events.clear()
    out = g.bloom(source=other, radius=5)
    assert [e if isinstance(e, str) else e[0] for e in g.events] == ["crender_bloom"]      # no push, no settle
    assert g.launches()[-1][2:] == (0, 33) and tuple(out.shape) == (33, 91, 3) and out is not other
    assert_bit_equal(out.numpy(), bloom_ref.bloom(other.numpy(), radius=5), "over the source")
    assert sorted(g._bloom_scratch) == [(33, 91), (70, 50)]
    assert not g._host_fresh and not g._host_exposed


def test_bloom_names_bad_arguments_before_anything_is_launched(hot):
    f = FakeFiller(hot)

    def refused(message, **kw):
        with pytest.raises(ValueError, match=message):
            f.bloom(**kw)

    for bad in (-1.0, NAN, "255", None, True):
        refused("threshold must be a number, 0 or above, got " + re.escape(repr(bad)), threshold=bad)
    for bad in (0, 33, -1, 8.0, True, None):
        refused("radius must be an int from 1 to 32, got " + re.escape(repr(bad)), radius=bad)
    for bad in ([1.0], [0.1] * 34, [[0.5, 0.5]], [0.5, NAN], [0.5, INF], "ab", 0.5):
        refused("weights must be a table of 2 to 33 finite numbers", weights=bad)
    for name in ("intensity", "exposure"):
        for bad in (-1.0, NAN, INF, 1e39, False, "2", None):
            refused(name + " must be a finite number, 0 or above, got " + re.escape(repr(bad)), **{name: bad})
    for bad in ("aces", "Reinhard", 1, True):
        refused("tonemap must be None, 'none' or 'reinhard', got " + re.escape(repr(bad)), tonemap=bad)
    for bad in (0, 0.0, -1.0, NAN, "1", None, True):
        refused("white must be a number above 0", white=bad)
    for bad in (0, 3, 2.2, True, None, "2"):
        refused("gamma must be 1 or 2, got " + re.escape(repr(bad)), gamma=bad)
    for bad in (NAN, "255", True):
        refused("clamp must be None or a number, got " + re.escape(repr(bad)), clamp=bad)
    for bad in ("float16", "u8", None, torch.uint8):
        refused("dtype must be 'float32' or 'uint8', got " + re.escape(repr(bad)), dtype=bad)
    good = torch.zeros((4, 5, 3))
    for bad in (good.numpy(), good.double(), good[:, :, :2], torch.zeros((4, 5)), torch.zeros((4, 5, 4)), good[:, ::2],
                torch.zeros((0, 5, 3)), good.permute(1, 0, 2)):
        refused("source must be a contiguous float32 \\[H, W, 3\\] device tensor", source=bad)
    assert f.events == []                                                 # nothing was pushed, settled or launched
    assert f._bloom_scratch is None
    f.device = "cuda:0"
    refused("source must be on the filler's device cuda:0, got cpu", source=good)
    from cython3dmodelrenderer_amd.pixel_buffer_filler import AdvancedPixelBufferFiller, EdgeOnlyPixelBufferFiller
    assert AdvancedPixelBufferFiller.bloom is DevicePlanes.bloom and EdgeOnlyPixelBufferFiller.bloom is DevicePlanes.bloom


def test_the_free_function_checks_its_image():
    from cython3dmodelrenderer_amd import bloom
    with pytest.raises(ValueError, match="image must be a contiguous float32"):
        bloom.bloom(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match=r"\['source'\] unknown"):
        bloom.bloom(torch.zeros((4, 4, 3)), source=None)
    with pytest.raises(ValueError, match="radius must be an int"):
        bloom.bloom(torch.zeros((4, 4, 3)), radius=0)
    with pytest.raises(ValueError, match="image must be on the device"):
        bloom.bloom(torch.zeros((4, 4, 3)))


# ---- the Renderer ----------------------------------------------------------------------------------------------

# a filler that records what the Renderer asks of it; each last pass returns a tensor of its own
IMAGES = {n: torch.full((8, 8, 3), float(i + 1)) for i, n in
          enumerate(("depth_of_field", "edge_aa", "transparency_pass", "resolve", "bloom"))}
_Recorder = recording_filler(
    "render_model set_fused_illumination wire_pass phong_pass ao_pass shade_guro depth_of_field edge_aa transparency_pass resolve bloom "
    "get_color_tensor get_color_buffer",
    returns=IMAGES, quiet="_push_host_edits synchronize get_normals_buffer", images=IMAGES)


def test_renderer_construction():
    from cython3dmodelrenderer_amd.renderer import Renderer
    params = list(inspect.signature(Renderer.__init__).parameters.values())
    names = [p.name for p in params]
    assert names[-4:] == ["bloom", "transparency", "wireframe", "supersample"] and params[-4].default is None
    assert names[names.index("bloom") - 1] == "environment"
    assert Renderer(SimpleNamespace(), None).bloom is None

    class Plain:
        pass
    with pytest.raises(ValueError, match=r"Renderer\(bloom=\.\.\.\) needs a filler that keeps its planes on the device.*Plain has no bloom"):
        Renderer(Plain(), None, bloom={})
    for key in ("source", "sigma", "tone"):
        with pytest.raises(ValueError, match=r"Renderer\(bloom=\.\.\.\) takes the keys 'threshold', .* and 'flip_rows': \['" + key + r"'\] unknown"):
            Renderer(_Recorder(), None, bloom={key: 1})
    opts = dict(threshold=200.0, radius=4, weights=None, intensity=0.5, exposure=2.0, tonemap="reinhard", white=3.0, gamma=2,
                clamp=255.0, dtype="uint8", flip_rows=True)
    r = Renderer(_Recorder(), None, bloom=opts)
    assert r.bloom == opts and r.bloom is not opts
    assert Renderer(_Recorder(), None, bloom={}).bloom == {}
    # the refusals among the four stay as they are
    f = _Recorder()
    with pytest.raises(ValueError, match="depth_of_field.*antialias.*supersample"):
        Renderer(f, None, bloom={}, depth_of_field=dict(focus=1.0), antialias={})
    with pytest.raises(ValueError, match="transparency.*antialias.*depth_of_field.*supersample"):
        Renderer(f, None, bloom={}, transparency=dict(alpha=0.5), supersample=2)
    with pytest.raises(ValueError, match="antialias.*supersample"):
        Renderer(f, None, bloom={}, antialias={}, supersample=2)


def test_renderer_runs_bloom_after_everything_else_over_the_last_pass_tensor():
    from cython3dmodelrenderer_amd.illumination import GuroIllumination, PhongIllumination
    from cython3dmodelrenderer_amd.renderer import Renderer
    model = SimpleNamespace(_vertices_by_triangles=np.zeros((1, 3, 3), np.float32))
    guro = GuroIllumination((0.3, -0.2, 1.0))
    opts = dict(threshold=200.0, radius=4)
    four = {"depth_of_field": ("depth_of_field", dict(focus=1.25)), "antialias": ("edge_aa", {}),
            "transparency": ("transparency_pass", dict(alpha=0.5)), "supersample": ("resolve", 2)}
    for keyword, (method, value) in four.items():
        for on_device in ("fused", True, None, False):
            f = _Recorder()
            got = Renderer(f, guro, on_device=on_device, bloom=opts, **{keyword: value}).render(model)
            names = f.names()
            assert names[-2:] == [method, "bloom"] and names.count("bloom") == 1 and names.count(method) == 1, (keyword, on_device)
            assert f.calls[-1][1] == () and f.calls[-1][2] == dict(source=f.images[method], **opts), (keyword, on_device)
            if on_device in ("fused", True):
                assert got is f.images["bloom"]
            else:
                assert isinstance(got, np.ndarray) and np.array_equal(got, f.images["bloom"].numpy())
    # alone: over the filler's own plane, which bloom completes itself; the frame is drawn as without it
    for on_device in ("fused", True, None, False):
        f, plain = _Recorder(), _Recorder()
        got = Renderer(f, guro, on_device=on_device, bloom=opts).render(model)
        Renderer(plain, guro, on_device=on_device).render(model)
        assert f.calls[:-1] == plain.calls and f.calls[-1] == ("bloom", (), dict(source=None, **opts)), on_device
        assert (got is f.images["bloom"]) if on_device in ("fused", True) else np.array_equal(got, f.images["bloom"].numpy())
    # a PhongIllumination with lines: the light, the lines, then bloom over the filler's plane; with a resolve over its tensor
    f = _Recorder()
    r = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), on_device=True, wireframe={}, bloom=opts)
    assert r.render(model) is f.images["bloom"] and r.render(model) is f.images["bloom"]
    assert f.names() == ["set_fused_illumination", "render_model", "phong_pass", "wire_pass", "get_color_tensor", "bloom"] * 2
    assert f.calls[-1][2]["source"] is None
    f = _Recorder()
    got = Renderer(f, PhongIllumination(position=(0.0, 0.0, 1.0)), supersample=2, bloom=opts).render(model)
    assert f.names()[-2:] == ["resolve", "bloom"] and f.calls[-1][2]["source"] is f.images["resolve"] and isinstance(got, np.ndarray)
    # without the option nothing changes
    f = _Recorder()
    assert Renderer(f, guro, on_device="fused").render(model) == "colour" and "bloom" not in f.names()
    f = _Recorder()
    assert Renderer(f, guro, on_device=True, depth_of_field=dict(focus=1.0)).render(model) is f.images["depth_of_field"]
    assert "bloom" not in f.names()
